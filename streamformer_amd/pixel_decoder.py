"""The Mask2Former pixel decoder on the HIP library: mask features and multi-scale features from the res2..res5 pyramid.

Mirror of the reference's ``MSDeformAttnPixelDecoder`` (``downstream/OVIS/mask2former/modeling/pixel_decoder/msdeformattn.py``), the consumer
of ``adapter.py``'s pyramid and of ``msda.py``'s operator in every shipped OVIS config.  The class carries the reference's explicit-keyword
constructor, parameter tree, state-dict keys and initialisation, so ``load_state_dict(strict=True)`` of the
``sem_seg_head.pixel_decoder.*`` slice of a CTVIS checkpoint works (the prefix is accepted and dropped); detectron2's ``Conv2d(norm=...)``
is restated as ``ConvNorm`` (``adapter_1.weight``, ``adapter_1.norm.weight``).  The forward runs in ``libstreamformer_hip.so``
(``sf_pixdec_forward``, kernels in ``csrc/sf_pixdec.hip``): no padding masks, no CPU fallback.

    dec = MSDeformAttnPixelDecoder({"res2": ShapeSpec(768, 4), ...}, transformer_dropout=0.0, transformer_nheads=8,
                                   transformer_dim_feedforward=1024, transformer_enc_layers=6, conv_dim=256, mask_dim=256, norm="GN",
                                   transformer_in_features=["res3", "res4", "res5"], common_stride=4).cuda().eval()
    mask_features, transformer_encoder_features, multi_scale_features = dec.forward_features(pyramid)

Training is an opt-in: ``trainable=True`` (constructor keyword or attribute, fp32 only) makes ``.train()`` run an autograd graph on the
module's own parameters instead of the refusal.  The graph stays in the rows layout [F, H W, C]: the 1 x 1 convolutions are ``F.linear``,
the 3 x 3 convolution is ``F.conv2d`` on the channels-last view of the rows, every GroupNorm (plain, with ReLU, with the FPN's
upsample-and-add) is one ``autograd.Function`` on ``sf_op_pixdec_groupnorm`` and its two backward entries (``csrc/sf_pixdec_bwd.hip``),
the sine table and the reference points are constants from ``sf_op_pixdec_pos_ref``, and each encoder layer calls its ``MSDeformAttn``
child (torch Linears around ``MSDeformAttnFunction``).  ``.eval()`` is the same native path either way; without the opt-in ``.train()``
is refused as before.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as TF
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as nat
from .msda import MSDeformAttn

__all__ = ["MSDeformAttnPixelDecoder", "ShapeSpec", "ConvNorm"]

PREFIX = "sem_seg_head.pixel_decoder."
ENC_N_POINTS = 4


@dataclass
class ShapeSpec:
    """The two fields of detectron2's ShapeSpec the decoder reads."""
    channels: int
    stride: int


def _c2_xavier_fill(conv: "ConvNorm") -> None:
    """fvcore's c2_xavier_fill: Caffe2's XavierFill is kaiming_uniform_ with a = 1; the bias is zero."""
    nn.init.kaiming_uniform_(conv.weight, a=1)
    if conv.bias is not None:
        nn.init.constant_(conv.bias, 0)


class ConvNorm(nn.Module):
    """A convolution's parameters with an optional ``norm`` child: the parameter tree of detectron2's ``Conv2d(..., norm=...)``."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, bias: bool = True, norm: Optional[nn.Module] = None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.norm = norm


class _EncoderLayer(nn.Module):
    def __init__(self, d_model: int, d_ffn: int, n_levels: int, n_heads: int, n_points: int, compute_dtype: Any):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points, compute_dtype=compute_dtype)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm2 = nn.LayerNorm(d_model)


class _Encoder(nn.Module):
    def __init__(self, layers: List[nn.Module]):
        super().__init__()
        self.layers = nn.ModuleList(layers)


class _EncoderOnly(nn.Module):
    """MSDeformAttnTransformerEncoderOnly's parameters (msdeformattn.py:23-53)."""

    def __init__(self, d_model: int, nhead: int, num_encoder_layers: int, dim_feedforward: int, num_feature_levels: int, compute_dtype: Any):
        super().__init__()
        self.encoder = _Encoder([_EncoderLayer(d_model, dim_feedforward, num_feature_levels, nhead, ENC_N_POINTS, compute_dtype)
                                 for _ in range(num_encoder_layers)])
        self.level_embed = nn.Parameter(torch.empty(num_feature_levels, d_model))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        nn.init.normal_(self.level_embed)


class _GroupNormFunction(Function):
    """GroupNorm(32, C) of rows ``x`` [F, H W, C] [+ ReLU] [+ the bilinear upsample of ``prev`` rows [F, Hp Wp, C]] on the HIP kernels.
    Saves ``x``, the statistics the forward wrote and the two parameters; not ``y``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, relu, size, prev, prev_size):
        Fr, HW, Cd = x.shape
        H, W = size
        Hp, Wp = prev_size if prev is not None else (0, 0)
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        prev_c = prev.contiguous() if prev is not None else None
        stats = torch.empty(Fr, 32, 4, device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        nat.launch(x.device, nat.lib.sf_op_pixdec_groupnorm, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), int(relu), nat.ptr(prev_c), Hp, Wp, None,
                   stats.data_ptr(), y.data_ptr(), None, None, None, None, Fr, H, W, Cd)
        ctx.save_for_backward(x, stats, gamma, beta)
        ctx.meta = (bool(relu), H, W, Hp, Wp, prev is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stats, gamma, beta = ctx.saved_tensors
        relu, H, W, Hp, Wp, has_prev = ctx.meta
        Fr, _, Cd = x.shape
        dev = x.device
        dy = dy.float().contiguous()
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dg = torch.empty_like(gamma) if need_g else None
        db = torch.empty_like(beta) if need_b else None
        if need_x or need_g or need_b:
            ws = nat.scratch(nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(Fr, H, W, Cd), dev)
            nat.launch(dev, nat.lib.sf_op_pixdec_groupnorm_backward, x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), int(relu),
                       dy.data_ptr(), nat.ptr(dx), nat.ptr(dg), nat.ptr(db), Fr, H, W, Cd, workspace=ws)
        d_prev = None
        if has_prev and ctx.needs_input_grad[5]:
            d_prev = torch.empty(Fr, Hp * Wp, Cd, device=dev, dtype=torch.float32)
            nat.launch(dev, nat.lib.sf_op_pixdec_upsample_backward, dy.data_ptr(), d_prev.data_ptr(), Fr, H, W, Hp, Wp, Cd)
        return dx, dg, db, None, None, d_prev, None


def _rows(x: torch.Tensor) -> torch.Tensor:
    """NCHW -> rows [F, H W, C], a view."""
    return x.flatten(2).transpose(1, 2)


def _nchw(rows: torch.Tensor, H: int, W: int) -> torch.Tensor:
    return rows.transpose(1, 2).reshape(rows.shape[0], rows.shape[2], H, W)


class MSDeformAttnPixelDecoder(nn.Module):
    """The reference's constructor plus ``compute_dtype`` ("fp32": bf16x3 operands, fp32-accurate; "bf16"), ``im2col_chunk_rows`` (pixels
    per gathered 3 x 3 operand, 0: the library's default) and ``trainable`` (also an attribute): with it ``.train()`` runs the autograd
    path of the module header (fp32 only, ``transformer_dropout`` must be 0), without it ``.train()`` is refused.  ``.eval()`` is the
    native forward in both cases."""

    def __init__(self, input_shape: Dict[str, Any], *, transformer_dropout: float, transformer_nheads: int, transformer_dim_feedforward: int,
                 transformer_enc_layers: int, conv_dim: int, mask_dim: int, norm: Any = None, transformer_in_features: List[str],
                 common_stride: int, compute_dtype: Any = "fp32", im2col_chunk_rows: int = 0, trainable: bool = False):
        super().__init__()
        self._compute = nat.compute_mode(compute_dtype)
        self.compute_dtype = compute_dtype
        self._trainable = False
        self.trainable = trainable
        if norm != "GN":
            raise NotImplementedError(f"norm {norm!r}: only norm=\"GN\" (GroupNorm(32, conv_dim)) runs natively")
        shapes = sorted(input_shape.items(), key=lambda kv: kv[1].stride)
        if not 1 <= len(shapes) <= 4:
            raise ValueError(f"input_shape names {len(shapes)} levels; the native decoder takes 1 to 4")
        self.in_features = [k for k, _ in shapes]
        self.feature_strides = [int(v.stride) for _, v in shapes]
        self.feature_channels = [int(v.channels) for _, v in shapes]
        self.transformer_in_features = [k for k in self.in_features if k in transformer_in_features]
        if not self.transformer_in_features:
            raise ValueError(f"transformer_in_features {list(transformer_in_features)} names no level of input_shape {self.in_features}")
        tr_channels = [c for k, c in zip(self.in_features, self.feature_channels) if k in self.transformer_in_features]
        self.transformer_feature_strides = [s for k, s in zip(self.in_features, self.feature_strides) if k in self.transformer_in_features]
        self.transformer_num_feature_levels = len(self.transformer_in_features)
        for name, value in (("conv_dim", conv_dim), ("transformer_dim_feedforward", transformer_dim_feedforward)):
            if value <= 0 or value % 64:
                raise ValueError(f"{name} = {value} must be a positive multiple of 64 (the GEMM kernels' k-step)")
        for k, ch in zip(self.in_features, self.feature_channels):
            if ch <= 0 or ch % 64:
                raise ValueError(f"input_shape[{k!r}].channels = {ch} must be a positive multiple of 64 (the GEMM kernels' k-step)")
        if transformer_nheads < 1 or conv_dim % transformer_nheads or (conv_dim // transformer_nheads) % 8 or not 8 <= conv_dim // transformer_nheads <= 128:
            raise ValueError(f"transformer_nheads = {transformer_nheads}: conv_dim / transformer_nheads must be a multiple of 8 in 8..128 "
                             "(deformable attention's channels per head)")
        if mask_dim < 4 or mask_dim % 4:
            raise ValueError(f"mask_dim = {mask_dim} must be a positive multiple of 4")
        self.conv_dim, self.mask_dim, self.common_stride = int(conv_dim), int(mask_dim), int(common_stride)
        self.nheads, self.dim_feedforward, self.enc_layers = int(transformer_nheads), int(transformer_dim_feedforward), int(transformer_enc_layers)
        self.transformer_dropout = float(transformer_dropout)            # never applied: the training path refuses a non-zero value
        self.im2col_chunk_rows = int(im2col_chunk_rows)
        self.maskformer_num_feature_levels = 3
        self.num_fpn_levels = int(math.log2(min(self.transformer_feature_strides)) - math.log2(self.common_stride))
        nat.OwnedHandle.release(self._create(0, nat.OwnedHandle(nat.lib.sf_pixdec_destroy, "pixel decoder probe")))      # the library's own rules, before any weight exists

        # from low resolution to high resolution (res5 -> res2), as the reference orders input_proj
        self.input_proj = nn.ModuleList([nn.Sequential(nn.Conv2d(ch, conv_dim, kernel_size=1), nn.GroupNorm(32, conv_dim))
                                         for ch in (tr_channels[::-1] if self.transformer_num_feature_levels > 1 else tr_channels[-1:])])
        for proj in self.input_proj:
            nn.init.xavier_uniform_(proj[0].weight, gain=1)
            nn.init.constant_(proj[0].bias, 0)
        self.transformer = _EncoderOnly(conv_dim, self.nheads, self.enc_layers, self.dim_feedforward, self.transformer_num_feature_levels, compute_dtype)
        self.mask_features = ConvNorm(conv_dim, mask_dim, 1)
        _c2_xavier_fill(self.mask_features)
        for idx, ch in enumerate(self.feature_channels[:self.num_fpn_levels]):
            lateral = ConvNorm(ch, conv_dim, 1, bias=False, norm=nn.GroupNorm(32, conv_dim))
            output = ConvNorm(conv_dim, conv_dim, 3, bias=False, norm=nn.GroupNorm(32, conv_dim))
            _c2_xavier_fill(lateral)
            _c2_xavier_fill(output)
            self.add_module(f"adapter_{idx + 1}", lateral)
            self.add_module(f"layer_{idx + 1}", output)
        self._native = nat.PackedHandle(self._create, nat.lib.sf_pixdec_load_tensor, self._finalize, nat.lib.sf_pixdec_destroy, "pixel decoder",
                                        dtype_of=_staged_dtype)

    # ------------------------------------------------------------------------------------ native handle
    def _create(self, device_index: int, h: Any = None):
        h = C.c_void_p() if h is None else h
        n = len(self.in_features)
        pad = lambda v: (C.c_int32 * 4)(*(list(v) + [0] * (4 - n)))      # noqa: E731
        cfg = nat.SfPixdecConfig(n, pad(self.feature_channels), pad(self.feature_strides),
                                 pad([int(k in self.transformer_in_features) for k in self.in_features]), self.conv_dim, self.mask_dim,
                                 self.nheads, self.dim_feedforward, self.enc_layers, ENC_N_POINTS, self.common_stride, 0, self.im2col_chunk_rows)
        nat.check(nat.lib.sf_pixdec_create(C.byref(cfg), device_index, C.byref(h)))
        return h

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_pixdec_finalize(h, self._compute))

    @property
    def device(self) -> torch.device:
        return self.mask_features.weight.device

    def _handle(self):
        """The native decoder, (re)packed when a parameter changed (in-place update, load_state_dict, .to(device))."""
        params = list(self.named_parameters())
        dev = self.device
        return self._native.get(dev, nat.weights_token(dev, [p for _, p in params]), params)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Keys with or without the checkpoint's leading ``sem_seg_head.pixel_decoder.``; with ``strict=False`` the rest of a whole
        checkpoint is ignored."""
        own = set(self.state_dict())
        sd = {}
        for k, v in state_dict.items():
            k2 = k[len(PREFIX):] if k.startswith(PREFIX) else k
            if strict or k2 in own:
                sd[k2] = v
        return super().load_state_dict(sd, strict=strict, assign=assign)

    # ------------------------------------------------------------------------------------ forward
    @property
    def trainable(self) -> bool:
        """Whether ``.train()`` runs the autograd path (fp32 only) instead of refusing."""
        return self._trainable

    @trainable.setter
    def trainable(self, value: bool) -> None:
        if value and self._compute != nat.compute_mode("fp32"):
            raise ValueError(f"trainable=True needs compute_dtype='fp32', got compute_dtype={self.compute_dtype!r} (there is no bf16 training mode)")
        self._trainable = bool(value)

    def forward_features(self, features: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
        """``features``: name -> fp32 (F, C_l, H_l, W_l) on the GPU.  Returns ``(mask_features, transformer_encoder_features,
        multi_scale_features)`` exactly as the reference's ``forward_features``: (F, mask_dim, H, W) of the finest level, the coarsest
        transformer level, and the first three entries of its ``out`` list.

        In ``.train()`` with ``trainable=True`` the three are differentiable in the module's parameters and in every level of
        ``features`` the decoder reads."""
        if self.training and not self._trainable:
            raise RuntimeError("the native pixel decoder is inference only: call .eval(), or opt in to the autograd path with trainable=True")
        if self.training:
            if self.transformer_dropout > 0:
                raise NotImplementedError(f"transformer_dropout = {self.transformer_dropout}: the training path applies no dropout (the shipped "
                                          "configs train with DROPOUT 0.0)")
            return self._forward_train(self._checked(features))
        with torch.no_grad():
            return self._forward_eval(self._checked(features))

    def _checked(self, features: Dict[str, torch.Tensor]) -> List[Optional[torch.Tensor]]:
        """Per input level the fp32 contiguous feature map on the module's device, None for a level the decoder does not read."""
        used = [k for i, k in enumerate(self.in_features) if k in self.transformer_in_features or i < self.num_fpn_levels]
        xs: List[Optional[torch.Tensor]] = []
        dev = self.device
        for k, ch in zip(self.in_features, self.feature_channels):
            if k not in used:
                xs.append(None)
                continue
            x = features[k]
            if x.device.type != "cuda" or dev.type != "cuda":
                raise RuntimeError("the pixel decoder runs on the MI355X: move the module and its inputs with .to('cuda') (there is no CPU fallback)")
            if x.dim() != 4 or x.shape[1] != ch:
                raise ValueError(f"features[{k!r}] must be (F, {ch}, H, W), got {tuple(x.shape)}")
            xs.append(x.to(device=dev, dtype=torch.float32).contiguous())
        live = [x for x in xs if x is not None]
        if any(x.shape[0] != live[0].shape[0] for x in live):
            raise ValueError("the levels of `features` hold different numbers of frames")
        return xs

    def _forward_train(self, xs: List[Optional[torch.Tensor]]) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
        dev = self.device
        Cd = self.conv_dim
        F = next(x for x in xs if x is not None).shape[0]
        tr = [i for i in range(len(xs) - 1, -1, -1) if self.in_features[i] in self.transformer_in_features]      # coarsest first
        L = len(tr)
        shapes = [tuple(xs[i].shape[2:]) for i in tr]
        starts = [sum(h * w for h, w in shapes[:j]) for j in range(L)]
        S = sum(h * w for h, w in shapes)

        def group_norm(rows, norm: nn.GroupNorm, size, relu=False, prev=None, prev_size=None):
            return _GroupNormFunction.apply(rows, norm.weight, norm.bias, relu, size, prev, prev_size)

        # the sine table and the reference points: constants, formed in fp64 and rounded once by the kernel (a zero level_embed)
        table = torch.empty(S, Cd, device=dev, dtype=torch.float32)
        ref = torch.empty(F, S, L, 2, device=dev, dtype=torch.float32)
        no_embed = torch.zeros(L, Cd, device=dev, dtype=torch.float32)      # level_embed[l] is added below, in torch, for its gradient
        nat.launch(dev, nat.lib.sf_op_pixdec_pos_ref, no_embed.data_ptr(), nat.i32_array([d for s in shapes for d in s]), L, F, Cd, table.data_ptr(),
                   ref.data_ptr())
        srcs, poss = [], []
        for j, l in enumerate(tr):
            conv, norm = self.input_proj[j][0], self.input_proj[j][1]
            srcs.append(group_norm(TF.linear(_rows(xs[l]), conv.weight.flatten(1), conv.bias), norm, shapes[j]))
            poss.append(table[starts[j]:starts[j] + shapes[j][0] * shapes[j][1]] + self.transformer.level_embed[j])
        src, pos = torch.cat(srcs, 1), torch.cat(poss, 0)
        for layer in self.transformer.encoder.layers:
            src = layer.norm1(src + layer.self_attn(src + pos, ref, src, shapes, starts))
            src = layer.norm2(src + layer.linear2(torch.relu(layer.linear1(src))))
        out = [(src[:, starts[j]:starts[j] + h * w], (h, w)) for j, (h, w) in enumerate(shapes)]
        for k in range(self.num_fpn_levels - 1, -1, -1):
            lateral, output = getattr(self, f"adapter_{k + 1}"), getattr(self, f"layer_{k + 1}")
            H, W = xs[k].shape[2:]
            prev, prev_size = out[-1]
            y = group_norm(TF.linear(_rows(xs[k]), lateral.weight.flatten(1)), lateral.norm, (H, W), prev=prev, prev_size=prev_size)
            y = TF.conv2d(y.view(F, H, W, Cd).permute(0, 3, 1, 2), output.weight, None, 1, 1)      # the rows ARE the channels-last image
            y = y.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(F, H * W, Cd)
            out.append((group_norm(y, output.norm, (H, W), relu=True), (H, W)))
        rows, (H, W) = out[-1]
        mask = _nchw(TF.linear(rows, self.mask_features.weight.flatten(1), self.mask_features.bias), H, W).contiguous()
        ms = [_nchw(r, h, w).contiguous() for r, (h, w) in out[:self.maskformer_num_feature_levels]]
        return mask, ms[0], ms

    def _forward_eval(self, xs: List[Optional[torch.Tensor]]) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
        dev = self.device
        F = next(x for x in xs if x is not None).shape[0]
        h = self._handle()
        n = len(xs)
        shapes = nat.i32_array([d for x in xs for d in ((x.shape[2], x.shape[3]) if x is not None else (1, 1))])
        n_ms = C.c_int()
        nat.check(nat.lib.sf_pixdec_num_outputs(h, C.byref(n_ms), None))
        out_levels = self.transformer_in_features[::-1] + self.in_features[:self.num_fpn_levels][::-1]
        by_name = dict(zip(self.in_features, xs))
        ms = [torch.empty(F, self.conv_dim, *by_name[k].shape[2:], dtype=torch.float32, device=dev) for k in out_levels[:n_ms.value]]
        mask = torch.empty(F, self.mask_dim, *by_name[out_levels[-1]].shape[2:], dtype=torch.float32, device=dev)
        ws = self._native.workspace(nat.sized(nat.lib.sf_pixdec_workspace_bytes, h, F, shapes, n), dev)
        nat.launch(dev, nat.lib.sf_pixdec_forward, h, nat.ptr_array(xs), F, shapes, n, mask.data_ptr(), nat.ptr_array(ms), len(ms), workspace=ws)
        return mask, ms[0], ms

    def forward(self, features: Dict[str, torch.Tensor], targets=None):
        return self.forward_features(features)


def _staged_dtype(dtype):
    """fp64 and bf16 tensors go to ``sf_pixdec_load_tensor`` as they are (it converts); everything else as fp32."""
    return {torch.float32: nat.SF_F32, torch.float64: nat.SF_F64, torch.bfloat16: nat.SF_BF16}.get(dtype)
