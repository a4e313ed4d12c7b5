"""The ViT-Adapter backbone on the MI355X: ``TimesformerMultiTaskingModelSigLIPViTAdapter``, a drop-in for the reference's class of the
same name (models/modeling_timesformer_siglip_adapter.py), for inference and, as an opt-in, for training under a frozen backbone.

It wraps the native encoder and returns the ``res2 .. res5`` feature pyramid (strides 4, 8, 16, 32) that the dense-prediction consumers
read (CTVIS / Mask2Former under downstream/OVIS).  Same constructor, parameter and buffer tree, state-dict keys and initialisation as the
reference; ``load_state_dict`` of a reference checkpoint works with ``strict=True``.

    from streamformer_amd import TimesformerMultiTaskingModelSigLIPViTAdapter
    model = TimesformerMultiTaskingModelSigLIPViTAdapter(config).to("cuda")
    model.load_state_dict(checkpoint)
    feats = model(pixel_values)            # [B, T, 3, H, W] -> {"res2", "res3", "res4", "res5"}: fp32 NCHW [B * T, D, ., .]

The forward path.  The residual stream stays frame-major ``[B, T, N, D]`` from ``sf_embed`` to the last ``sf_layers``: that IS the
``[B * T, N, D]`` the extractors read, so the reference's permutes between its patch-major stream and the extractors (adapter:426-430,
645-649) do not exist here.  Per interaction block ``sf_layers(begin, end + 1)`` runs in place, then one extractor (three after the last
block): ``sf_op_layernorm`` on query and feature, ``MSDeformAttn``'s no-grad path with the residual added by the output GEMM,
``sf_op_layernorm``, and the ConvFFN as ``sf_op_linear`` -> ``sf_op_adapter_dwconv_gelu`` -> ``sf_op_linear`` (+ residual).  The tail is one
GEMM for ``ConvTranspose2d(D, D, 2, 2)`` and ``sf_op_adapter_fuse`` per level (tokens + bilinear ViT feature [+ c1] + eval BatchNorm,
written NCHW).  The spatial prior module (the 3 x 3 convolution stem, about 5 % of the FLOPs at SigLIP-base) stays torch.

Inference by default: ``eval()`` mode, ``SyncBatchNorm`` as its running-statistics affine, outputs carry no graph; ``forward`` in training
mode raises unless the module was built (or later marked) ``trainable=True``.

Training is an opt-in: ``trainable=True`` (constructor keyword or attribute, fp32 only) makes ``.train()`` run an autograd graph on the
module's own parameters under a FROZEN backbone, which is how the reference trains this module (``freeze_backbone=True``).  The spatial
prior module runs in torch with its ``SyncBatchNorm`` layers in training mode (batch statistics, running statistics updated, synchronised
across ranks by torch when a process group exists), ``sf_embed`` / ``sf_layers`` run without a graph exactly as in ``eval()`` (``feat`` and
the kept ViT maps are constants, no gradient passes through an encoder layer), every extractor is ``F.layer_norm`` / ``F.linear`` /
``MSDeformAttn``'s autograd path plus one ``autograd.Function`` for DWConv + GELU (forward: the inference kernel, backward:
``sf_op_adapter_dwconv_gelu_backward``; saves x, w, b, not y), and the tail is ``F.linear`` on a view of ``up.weight``, one
``autograd.Function`` per level on ``sf_op_adapter_fuse`` (unit scale, zero shift) and ``sf_op_adapter_fuse_backward``, and ``norm1..4``
as the torch modules they are.  A parameter of the backbone that requires a gradient, a non-zero dropout or drop-path rate in the config
and ``with_cp=True`` are refused by name before anything runs.  ``eval()`` of a ``trainable=True`` module is the inference path, bit for bit.

``conv_inplane`` and ``deform_ratio`` are accepted and ignored exactly as the reference does (it builds
``SpatialPriorModule(inplanes=64)`` and its live ``MSDeformAttn`` ignores ``ratio``); ``init_values``, ``finetune`` and
``finetune_indexes`` are unused there too (the injector they belonged to is commented out).  The reference's adapter has no ``head``: the
inner native encoder keeps a default-initialised one that is never run and is not part of this module's ``state_dict()``.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Any, Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as nat
from .configuration import StreamformerConfig
from .modeling import TimesformerMultiTaskingModelSigLIP
from .msda import MSDeformAttn, _Levels

__all__ = ["TimesformerMultiTaskingModelSigLIPViTAdapter"]

_OUTPUTS = ("res2", "res3", "res4", "res5")


class SpatialPriorModule(nn.Module):
    """adapter:106-208 — the convolution stem; runs in torch."""

    def __init__(self, inplanes: int = 64, embed_dim: int = 384):
        super().__init__()

        def conv(ci, co, stride):
            return [nn.Conv2d(ci, co, kernel_size=3, stride=stride, padding=1, bias=False), nn.SyncBatchNorm(co), nn.ReLU(inplace=True)]

        self.stem = nn.Sequential(*conv(3, inplanes, 2), *conv(inplanes, inplanes, 1), *conv(inplanes, inplanes, 1),
                                  nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        self.conv2 = nn.Sequential(*conv(inplanes, 2 * inplanes, 2))
        self.conv3 = nn.Sequential(*conv(2 * inplanes, 4 * inplanes, 2))
        self.conv4 = nn.Sequential(*conv(4 * inplanes, 4 * inplanes, 2))
        self.fc1 = nn.Conv2d(inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc2 = nn.Conv2d(2 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc3 = nn.Conv2d(4 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc4 = nn.Conv2d(4 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)

    def forward(self, x: torch.Tensor):
        c1 = self.stem(x)
        c2 = self.conv2(c1)
        c3 = self.conv3(c2)
        c4 = self.conv4(c3)
        return self.fc1(c1), self.fc2(c2), self.fc3(c3), self.fc4(c4)


class DWConv(nn.Module):
    def __init__(self, dim: int = 768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)


class ConvFFN(nn.Module):
    def __init__(self, in_features: int, hidden_features: int):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.drop = nn.Dropout(0.0)


class Extractor(nn.Module):
    """adapter:257-316 — parameters only; the adapter's forward runs it."""

    def __init__(self, dim: int, num_heads: int, n_points: int, deform_ratio: float, with_cffn: bool, cffn_ratio: float, eps: float,
                 compute_dtype: Any):
        super().__init__()
        self.query_norm = nn.LayerNorm(dim, eps=eps)
        self.feat_norm = nn.LayerNorm(dim, eps=eps)
        self.attn = MSDeformAttn(d_model=dim, n_levels=1, n_heads=num_heads, n_points=n_points, ratio=deform_ratio, compute_dtype=compute_dtype)
        self.with_cffn = with_cffn
        if with_cffn:
            self.ffn = ConvFFN(in_features=dim, hidden_features=int(dim * cffn_ratio))
            self.ffn_norm = nn.LayerNorm(dim, eps=eps)
            self.drop_path = nn.Identity()


class InteractionBlock(nn.Module):
    def __init__(self, extra_extractor: bool, **kw):
        super().__init__()
        self.extractor = Extractor(**kw)
        self.extra_extractors = nn.Sequential(*[Extractor(**kw) for _ in range(2)]) if extra_extractor else None

    def extractors(self) -> List[Extractor]:
        return [self.extractor] + (list(self.extra_extractors) if self.extra_extractors is not None else [])


class _DWConvGeluFunction(Function):
    """ConvFFN's DWConv + GELU on the three-level tokens ``x`` [F, 21 n, C] on the HIP kernels.  Saves ``x``, ``w`` and ``b``, not ``y``: the
    backward recomputes the convolution."""

    @staticmethod
    def forward(ctx, x, w, b, Hg, Wg):
        x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
        y = torch.empty_like(x)
        nat.launch(x.device, nat.lib.sf_op_adapter_dwconv_gelu, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), x.shape[0], Hg, Wg, x.shape[2])
        ctx.save_for_backward(x, w, b)
        ctx.grid = (Hg, Wg)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        Hg, Wg = ctx.grid
        Fr, _, Cd = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        dy = dy.float().contiguous()
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty_like(b) if need_b else None
        ws = nat.scratch(nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(Fr, Hg, Wg, Cd), x.device)
        nat.launch(x.device, nat.lib.sf_op_adapter_dwconv_gelu_backward, x.data_ptr(), w.data_ptr(), b.data_ptr(), dy.data_ptr(), nat.ptr(dx), nat.ptr(dw),
                   nat.ptr(db), Fr, Hg, Wg, Cd, workspace=ws)
        return dx, dw, db, None, None


class _FuseFunction(Function):
    """One level of the tail without its BatchNorm: ``tokens`` (level 0: the transposed convolution's GEMM output [F, 16 n, 4 D]; levels
    1..3: the level's slice of ``c``, [F, pixels, D] with any frame stride) + the bilinear resampling of the constant ViT map ``vit`` [+ c1],
    written NCHW by ``sf_op_adapter_fuse`` with the unit scale ``one`` and the zero shift ``zero``.  The backward is a re-layout of dy
    (``sf_op_adapter_fuse_backward``), and dy itself for c1."""

    @staticmethod
    def forward(ctx, tokens, c1, vit, one, zero, level, Hg, Wg):
        Fr, D = tokens.shape[0], one.shape[0]
        if tokens.stride(2) != 1 or tokens.stride(1) != tokens.shape[2] or tokens.stride(0) % 4 or tokens.data_ptr() % 16:
            tokens = tokens.contiguous()
        c1 = c1.contiguous() if c1 is not None else None
        out = torch.empty(Fr, D, *Ho_Wo(level, Hg, Wg), dtype=torch.float32, device=tokens.device)
        nat.launch(tokens.device, nat.lib.sf_op_adapter_fuse, level, tokens.data_ptr(), tokens.stride(0), nat.ptr(vit), nat.ptr(c1), one.data_ptr(),
                   zero.data_ptr(), out.data_ptr(), Fr, Hg, Wg, D)
        ctx.meta = (level, Hg, Wg, D, tuple(tokens.shape))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        level, Hg, Wg, D, shape = ctx.meta
        dy = dy.float().contiguous()
        d_tok = None
        if ctx.needs_input_grad[0]:
            d_tok = torch.empty(shape, dtype=torch.float32, device=dy.device)
            nat.launch(dy.device, nat.lib.sf_op_adapter_fuse_backward, level, dy.data_ptr(), d_tok.data_ptr(), shape[1] * shape[2], shape[0], Hg, Wg, D)
        return d_tok, (dy if level == 0 and ctx.needs_input_grad[1] else None), None, None, None, None, None, None


def _check_partition(indexes: Sequence[Sequence[int]], layers: int) -> None:
    nxt = 0
    for pair in indexes:
        if len(pair) != 2 or int(pair[0]) != nxt or int(pair[1]) < int(pair[0]):
            raise ValueError(f"interaction_indexes {list(map(list, indexes))} must split the layers 0 .. {layers - 1} into consecutive [begin, end] ranges")
        nxt = int(pair[1]) + 1
    if nxt != layers:
        raise ValueError(f"interaction_indexes {list(map(list, indexes))} must split the layers 0 .. {layers - 1} into consecutive [begin, end] ranges")


class TimesformerMultiTaskingModelSigLIPViTAdapter(nn.Module):
    """MI355X-native stand-in for the reference class of the same name (adapter:454-680)."""

    config_class = StreamformerConfig
    base_model_prefix = "timesformer"
    main_input_name = "pixel_values"

    def __init__(self, config: StreamformerConfig = None, pretrain_size: int = 224, conv_inplane: int = 64, n_points: int = 4,
                 deform_num_heads: int = 12, init_values: float = 1e-6, interaction_indexes=[[0, 2], [3, 5], [6, 8], [9, 11]],
                 with_cffn: bool = True, cffn_ratio: float = 0.25, deform_ratio: float = 0.5, add_vit_feature: bool = True,
                 use_extra_extractor: bool = True, with_cp: bool = False, freeze_backbone: bool = True, finetune: bool = False,
                 finetune_indexes=[0], compute_dtype: Any = "fp32", trainable: bool = False):
        super().__init__()
        config = StreamformerConfig() if config is None else config
        D = config.hidden_size
        # every refusal happens here or at the top of forward(): before anything is built or launched
        if config.patch_size != 16:
            raise NotImplementedError(f"patch_size={config.patch_size}: the adapter views the stride-16 level as the patch grid (adapter:656), which "
                                      "needs patch_size 16")
        if with_cp:
            raise NotImplementedError("with_cp=True: activation checkpointing is not implemented, neither for inference nor for the trainable=True path")
        if D % 64:
            raise ValueError(f"hidden_size={D} must be a multiple of 64 (the GEMM kernels' k-step)")
        if with_cffn and (int(D * cffn_ratio) < 64 or int(D * cffn_ratio) % 64):
            raise ValueError(f"cffn_ratio={cffn_ratio}: the ConvFFN width int(hidden_size * cffn_ratio) = {int(D * cffn_ratio)} must be a multiple of 64 "
                             "(the GEMM kernels' k-step)")
        if deform_num_heads < 1 or D % deform_num_heads or (D // deform_num_heads) % 8 or not 8 <= D // deform_num_heads <= 128:
            raise ValueError(f"deform_num_heads={deform_num_heads}: hidden_size / deform_num_heads must be a whole multiple of 8 in 8..128 "
                             f"(the deformable-attention kernel's head widths), hidden_size is {D}")
        if not 1 <= n_points <= 8:
            raise ValueError(f"n_points={n_points} outside 1..8 (the deformable-attention kernel's limit)")
        _check_partition(interaction_indexes, config.num_hidden_layers)
        if add_vit_feature and len(interaction_indexes) != 4:
            raise ValueError(f"interaction_indexes has {len(interaction_indexes)} blocks: add_vit_feature=True adds the ViT features of exactly four "
                             "(adapter:661)")
        self._compute = nat.compute_mode(compute_dtype)
        self.compute_dtype = compute_dtype
        self._trainable = False
        self.trainable = trainable
        self.config = config
        self.add_vit_feature, self.freeze_backbone = bool(add_vit_feature), bool(freeze_backbone)
        self.interaction_indexes = [[int(a), int(b)] for a, b in interaction_indexes]
        self.num_blocks = config.num_hidden_layers

        # the native encoder owns embeddings / encoder / post_layernorm (and a head this module never runs); its three containers are
        # registered here under the reference's names, so they are this module's parameters and state-dict entries too
        enc = TimesformerMultiTaskingModelSigLIP(config, compute_dtype=compute_dtype)
        object.__setattr__(self, "_enc", enc)
        self.embeddings, self.encoder, self.post_layernorm = enc.embeddings, enc.encoder, enc.post_layernorm

        self.level_embed = nn.Parameter(torch.zeros(3, D))
        self.spm = SpatialPriorModule(inplanes=64, embed_dim=D)
        kw = dict(dim=D, num_heads=deform_num_heads, n_points=n_points, deform_ratio=deform_ratio, with_cffn=with_cffn, cffn_ratio=cffn_ratio,
                  eps=config.layer_norm_eps, compute_dtype=compute_dtype)
        last = len(interaction_indexes) - 1
        self.interactions = nn.Sequential(*[InteractionBlock(extra_extractor=(i == last and use_extra_extractor), **kw) for i in range(last + 1)])
        self.up = nn.ConvTranspose2d(D, D, 2, 2)
        self.norm1, self.norm2, self.norm3, self.norm4 = (nn.SyncBatchNorm(D) for _ in range(4))

        # one workspace for every GEMM of the adapter (the extractors' MSDeformAttn modules share it), the folded tail, the geometry
        self._native = nat.PackedHandle(noun="ViT-Adapter")
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._native = self._native
        self._tail, self._tail_token = None, None
        self._unit = None                    # the training path's (unit scale, zero shift) of sf_op_adapter_fuse
        self._geometry: Dict[tuple, tuple] = {}
        self._marks = None                   # tools/vit_adapter_bench.py: a list that receives (stage, HIP event) pairs during a forward

        self._init_adapter_weights()
        if self.freeze_backbone:
            for part in (self.encoder, self.embeddings, self.post_layernorm):
                for p in part.parameters():
                    p.requires_grad = False
        self.eval()

    # --------------------------------------------------------------------------------- initialisation
    @staticmethod
    def _init_weights(m: nn.Module) -> None:
        """adapter:556-570."""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, nn.BatchNorm2d)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
            m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
            if m.bias is not None:
                m.bias.data.zero_()

    def _init_adapter_weights(self) -> None:
        """The reference's sequence (adapter:529-544): ``_init_weights`` over up, spm and interactions, ``MSDeformAttn._reset_parameters``,
        ``normal_(level_embed)``, then ``post_init()`` — which applies ``_init_weights`` to every module once more, so the deformable
        attention's four Linears end as every other Linear does (truncated normal 0.02, zero bias).  The encoder keeps its own rules."""
        adapter_parts = (self.up, self.spm, self.interactions)
        for part in adapter_parts:
            part.apply(self._init_weights)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        nn.init.normal_(self.level_embed)
        for part in adapter_parts:
            part.apply(self._init_weights)

    # ------------------------------------------------------------------------------ module surface
    def _apply(self, fn, recurse: bool = True):
        out = super()._apply(fn, recurse)
        self._enc._apply(fn)                 # the head the encoder keeps, and its own bookkeeping (packed weights, workspaces)
        self._native.workspaces.clear()
        self._tail_token = None
        self._unit = None
        self._geometry.clear()
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        res = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if assign:
            self._enc._refresh_plist()
        self._enc.refresh_weights()
        self._tail_token = None
        return res

    def train(self, mode: bool = True):
        super().train(mode)
        self._enc.training = mode
        return self

    @property
    def trainable(self) -> bool:
        """Whether ``.train()`` runs the autograd path (fp32 only, frozen backbone) instead of refusing."""
        return self._trainable

    @trainable.setter
    def trainable(self, value: bool) -> None:
        if value and self._compute != nat.SF_COMPUTE_BF16X3:
            raise ValueError(f"trainable=True needs compute_dtype='fp32', got compute_dtype={self.compute_dtype!r} (there is no bf16 training mode)")
        self._trainable = bool(value)

    def _check_trainable(self) -> None:
        """What ``.train()`` refuses, by name, before anything runs."""
        if not self._trainable:
            raise NotImplementedError("the native ViT-Adapter is inference only (SyncBatchNorm as its running statistics, no gradients): call .eval(), "
                                      "or opt in to the autograd path under a frozen backbone with trainable=True")
        for part in ("embeddings", "encoder", "post_layernorm"):
            for k, p in getattr(self, part).named_parameters():
                if p.requires_grad:
                    raise NotImplementedError(f"{part}.{k} requires a gradient (freeze_backbone={self.freeze_backbone}): the trainable=True path trains the "
                                              "adapter under a frozen backbone, no gradient passes through an encoder layer")
        for field in ("hidden_dropout_prob", "attention_probs_dropout_prob", "drop_path_rate"):
            if float(getattr(self.config, field, 0.0) or 0.0) != 0.0:
                raise NotImplementedError(f"config.{field}={getattr(self.config, field)}: the frozen encoder runs its inference kernels, which have no "
                                          "dropout or drop path; set it to 0")

    def get_input_embeddings(self):
        return self.embeddings.patch_embeddings

    @property
    def device(self) -> torch.device:
        return self.level_embed.device

    def __getstate__(self):
        return dict(self.__dict__, _tail=None, _tail_token=None, _unit=None, _geometry={}, _marks=None)

    def _mark(self, stage: str) -> None:
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((stage, ev))

    # ------------------------------------------------------------------------------- native pieces
    def _layernorm(self, x: torch.Tensor, ln: nn.LayerNorm) -> torch.Tensor:
        y = torch.empty_like(x)
        nat.launch(x.device, nat.lib.sf_op_layernorm, x.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), y.data_ptr(), x.numel() // x.shape[-1],
                   x.shape[-1], float(ln.eps))
        return y

    def _linear(self, x: torch.Tensor, w: torch.Tensor, b, resid=None) -> torch.Tensor:
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        ws = self._native.workspace(nat.lib.sf_op_linear_workspace_bytes(M, N, K), x.device)
        nat.launch(x.device, nat.lib.sf_op_linear, x.data_ptr(), w.data_ptr(), nat.ptr(b), nat.ptr(resid), 1.0, 0, y.data_ptr(), M, N, K, self._compute,
                   workspace=ws)
        return y

    def _extract(self, ex: Extractor, c: torch.Tensor, feat: torch.Tensor, ref: torch.Tensor, lv: _Levels, Hg: int, Wg: int) -> torch.Tensor:
        """Extractor.forward (adapter:295-309) on c [F, 21 n, D] and feat [F, N, D]."""
        Fr, Lq, D = c.shape
        c = ex.attn._forward_native(self._layernorm(c, ex.query_norm), ref, self._layernorm(feat, ex.feat_norm), lv, None, resid=c)
        if not ex.with_cffn:
            return c
        ffn = ex.ffn
        u = self._linear(self._layernorm(c, ex.ffn_norm).view(Fr * Lq, D), ffn.fc1.weight, ffn.fc1.bias)
        v = torch.empty_like(u)
        nat.launch(c.device, nat.lib.sf_op_adapter_dwconv_gelu, u.data_ptr(), ffn.dwconv.dwconv.weight.data_ptr(), ffn.dwconv.dwconv.bias.data_ptr(),
                   v.data_ptr(), Fr, Hg, Wg, u.shape[1])
        return self._linear(v, ffn.fc2.weight, ffn.fc2.bias, resid=c.view(Fr * Lq, D)).view(Fr, Lq, D)

    def _folded_tail(self, dev) -> Tuple[torch.Tensor, List[torch.Tensor], List[torch.Tensor]]:
        """The transposed convolution as a Linear weight [(dy, dx, c_out), c_in] and the four eval BatchNorms as (scale, shift), up.bias folded
        into norm1's shift; rebuilt when one of their tensors changes."""
        norms = [self.norm1, self.norm2, self.norm3, self.norm4]
        ps = [self.up.weight, self.up.bias] + [t for n in norms for t in (n.weight, n.bias, n.running_mean, n.running_var)]
        token = nat.weights_token(dev, ps)
        if token != self._tail_token:
            with torch.no_grad():
                D = self.up.weight.shape[0]
                up_w = self.up.weight.float().permute(2, 3, 1, 0).reshape(4 * D, D).contiguous()
                scales, shifts = [], []
                for i, n in enumerate(norms):
                    scale = n.weight.double() / torch.sqrt(n.running_var.double() + n.eps)
                    shift = n.bias.double() - n.running_mean.double() * scale
                    if i == 0:
                        shift = shift + scale * self.up.bias.double()
                    scales.append(scale.float().contiguous())
                    shifts.append(shift.float().contiguous())
            self._tail, self._tail_token = (up_w, scales, shifts), token
        return self._tail

    def _geometry_for(self, Fr: int, Hg: int, Wg: int, dev) -> Tuple[torch.Tensor, _Levels]:
        """Reference points of the three query levels (get_reference_points, adapter:19-32: fp32 cell centres) for every frame, and the level
        table of the one value level: built once per (frames, grid, device)."""
        key = (Fr, Hg, Wg, dev)
        hit = self._geometry.get(key)
        if hit is None:
            pts = []
            for H_, W_ in ((2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2)):
                ys = torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32) / H_
                xs = torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32) / W_
                ry, rx = torch.meshgrid(ys, xs, indexing="ij")
                pts.append(torch.stack((rx.reshape(-1), ry.reshape(-1)), -1))
            ref = torch.cat(pts, 0)[None, :, None, :].expand(Fr, -1, -1, -1).contiguous().to(dev)
            hit = self._geometry[key] = (ref, _Levels([(Hg, Wg)]))
        return hit

    # ------------------------------------------------------------------------ the training path
    def _extract_train(self, ex: Extractor, c: torch.Tensor, feat: torch.Tensor, ref: torch.Tensor, lv: _Levels, Hg: int, Wg: int) -> torch.Tensor:
        """``_extract`` as a graph of torch operators on the extractor's parameters; ``feat`` is a constant."""
        c = c + ex.attn._forward_autograd(ex.query_norm(c), ref, ex.feat_norm(feat), lv, None)
        if not ex.with_cffn:
            return c
        ffn = ex.ffn
        u = ffn.fc1(ex.ffn_norm(c))
        v = _DWConvGeluFunction.apply(u, ffn.dwconv.dwconv.weight, ffn.dwconv.dwconv.bias, Hg, Wg)
        return c + ffn.fc2(v)

    def _forward_train(self, pixel_values: torch.Tensor) -> Tuple["OrderedDict[str, torch.Tensor]", torch.Tensor]:
        dev, enc, D = self.device, self._enc, self.config.hidden_size
        B, T, _, H, W = pixel_values.shape
        Fr, Hg, Wg = B * T, H // 16, W // 16
        n = (Hg // 2) * (Wg // 2)
        x = pixel_values.detach().to(dev, torch.float32).contiguous()
        self._mark("start")
        cd = torch.backends.cudnn              # the deterministic convolution algorithms, as in eval()
        with cd.flags(enabled=cd.enabled, benchmark=cd.benchmark, deterministic=True, allow_tf32=cd.allow_tf32):
            c1, c2, c3, c4 = self.spm(x.view(Fr, 3, H, W))
        le = self.level_embed
        c = torch.cat([t.flatten(2).transpose(1, 2) + le[i] for i, t in enumerate((c2, c3, c4))], 1)
        self._mark("spm")
        ref, lv = self._geometry_for(Fr, Hg, Wg, dev)
        kept: List[torch.Tensor] = []
        last = len(self.interactions) - 1
        with torch.no_grad():
            ws = enc._stage_ws(B, T, H, W)
            handle = enc._handle
            h = torch.empty(B, T, Hg * Wg, D, dtype=torch.float32, device=dev)
            nat.launch(dev, nat.lib.sf_embed, handle, x.data_ptr(), nat.SF_F32, B, T, H, W, h.data_ptr(), nat.ptr(enc._pos_table(H, W)), workspace=ws)
        self._mark("embed")
        for i, (block, (la, lb)) in enumerate(zip(self.interactions, self.interaction_indexes)):
            with torch.no_grad():
                nat.launch(dev, nat.lib.sf_layers, handle, h.data_ptr(), B, T, H, W, la, lb + 1, None, workspace=ws)
                # the graph keeps this block's stream (LayerNorm's input), and sf_layers goes on in place: every block but the last gets a copy
                feat = h.view(Fr, Hg * Wg, D) if i == last else h.view(Fr, Hg * Wg, D).clone()
            self._mark("layers")
            for ex in block.extractors():
                c = self._extract_train(ex, c, feat, ref, lv, Hg, Wg)
            kept.append(feat)
            self._mark("extractors")
        if self._unit is None or self._unit[0].device != dev or self._unit[0].shape[0] != D:
            self._unit = (torch.ones(D, dtype=torch.float32, device=dev), torch.zeros(D, dtype=torch.float32, device=dev))
        one, zero = self._unit
        up_w = self.up.weight.permute(2, 3, 1, 0).reshape(4 * D, D)
        up = F.linear(c[:, :16 * n], up_w, self.up.bias.repeat(4))                # [F, 16 n, 4 D]: columns (dy, dx, c_out)
        toks = (up, c[:, :16 * n], c[:, 16 * n:20 * n], c[:, 20 * n:])
        outs = OrderedDict()
        for level, (name, norm) in enumerate(zip(_OUTPUTS, (self.norm1, self.norm2, self.norm3, self.norm4))):
            pre = _FuseFunction.apply(toks[level], c1 if level == 0 else None, kept[level] if self.add_vit_feature else None, one, zero, level, Hg, Wg)
            outs[name] = norm(pre)
        self._mark("tail")
        return outs, c

    # ------------------------------------------------------------------------------------ forward
    def forward(self, pixel_values: torch.Tensor, output_attentions=None, output_hidden_states=None, return_dict=None) -> "OrderedDict[str, torch.Tensor]":
        """pixel_values [B, T, 3, H, W] (H, W multiples of 32) -> {"res2", "res3", "res4", "res5"}: fp32 NCHW [B * T, D, H / s, W / s] at
        s = 4, 8, 16, 32, in the reference's key order.  The three flags are accepted and unused, as in the reference."""
        return self.forward_with_tokens(pixel_values)[0]

    def forward_with_tokens(self, pixel_values: torch.Tensor) -> Tuple["OrderedDict[str, torch.Tensor]", torch.Tensor]:
        """``forward`` and the extractors' final tokens ``c`` [B * T, 21 n, D] (the three levels at strides 8, 16, 32, before the tail)."""
        if self.training:
            self._check_trainable()
        if pixel_values.dim() != 5 or pixel_values.shape[2] != self.config.num_channels:
            raise ValueError(f"pixel_values must be (B, T, {self.config.num_channels}, H, W), got {tuple(pixel_values.shape)}")
        B, T, _, H, W = pixel_values.shape
        if H % 32 or W % 32 or H < 32 or W < 32:
            raise ValueError(f"pixel_values: H = {H} and W = {W} must be multiples of 32 (the stride-32 level halves the patch grid)")
        dev = self.device
        if dev.type != "cuda" or pixel_values.device.type != "cuda":
            raise RuntimeError("the ViT-Adapter runs on the MI355X: move the module and its input with .to('cuda') (there is no CPU fallback)")
        if self.level_embed.dtype != torch.float32:
            raise TypeError(f"the ViT-Adapter keeps fp32 parameters (compute_dtype picks the GEMM precision), got {self.level_embed.dtype}")
        if self.training:
            with torch.cuda.device(dev):
                return self._forward_train(pixel_values)
        enc, D = self._enc, self.config.hidden_size
        Fr, Hg, Wg = B * T, H // 16, W // 16
        n = (Hg // 2) * (Wg // 2)
        with torch.no_grad(), torch.cuda.device(dev):
            x = pixel_values.to(dev, torch.float32).contiguous()
            self._mark("start")
            # spatial prior module (torch): c1 NCHW, c2..c4 as tokens with their level embedding
            # deterministic convolution algorithms: the default choice for the stride-2 convolutions sums in arrival order, and the
            # extractors amplify its last-bit differences a hundredfold; with them the whole forward is bit-reproducible
            cd = torch.backends.cudnn
            with cd.flags(enabled=cd.enabled, benchmark=cd.benchmark, deterministic=True, allow_tf32=cd.allow_tf32):
                c1, c2, c3, c4 = self.spm(x.view(Fr, 3, H, W).to(self.level_embed.dtype))
            le = self.level_embed
            c = torch.cat([t.flatten(2).transpose(1, 2) + le[i] for i, t in enumerate((c2, c3, c4))], 1).float().contiguous()
            c1 = c1.float().contiguous()
            self._mark("spm")
            # embeddings, then the encoder layers in groups on the frame-major stream
            ws = enc._stage_ws(B, T, H, W)
            handle = enc._handle
            h = torch.empty(B, T, Hg * Wg, D, dtype=torch.float32, device=dev)
            nat.launch(dev, nat.lib.sf_embed, handle, x.data_ptr(), nat.SF_F32, B, T, H, W, h.data_ptr(), nat.ptr(enc._pos_table(H, W)), workspace=ws)
            self._mark("embed")
            ref, lv = self._geometry_for(Fr, Hg, Wg, dev)
            feat = h.view(Fr, Hg * Wg, D)
            kept: List[torch.Tensor] = []
            last = len(self.interactions) - 1
            for i, (block, (la, lb)) in enumerate(zip(self.interactions, self.interaction_indexes)):
                nat.launch(dev, nat.lib.sf_layers, handle, h.data_ptr(), B, T, H, W, la, lb + 1, None, workspace=ws)
                self._mark("layers")
                for ex in block.extractors():
                    c = self._extract(ex, c, feat, ref, lv, Hg, Wg)
                if self.add_vit_feature:
                    kept.append(feat if i == last else feat.clone())
                self._mark("extractors")
            # tail: transposed convolution as a GEMM, then one fusion kernel per level
            up_w, scales, shifts = self._folded_tail(dev)
            frame = 21 * n * D
            up = self._linear(c[:, :16 * n].reshape(Fr * 16 * n, D), up_w, None)
            outs = OrderedDict()
            for level, (name, tok, stride) in enumerate(zip(_OUTPUTS, (up.data_ptr(), c.data_ptr(), c.data_ptr() + 4 * 16 * n * D,
                                                                       c.data_ptr() + 4 * 20 * n * D), (16 * n * 4 * D, frame, frame, frame))):
                out = torch.empty(Fr, D, *Ho_Wo(level, Hg, Wg), dtype=torch.float32, device=dev)
                nat.launch(dev, nat.lib.sf_op_adapter_fuse, level, tok, stride, nat.ptr(kept[level]) if self.add_vit_feature else None,
                           c1.data_ptr() if level == 0 else None, scales[level].data_ptr(), shifts[level].data_ptr(), out.data_ptr(), Fr, Hg, Wg, D)
                outs[name] = out
            self._mark("tail")
        return outs, c


def Ho_Wo(level: int, Hg: int, Wg: int) -> Tuple[int, int]:
    """The output grid of pyramid level 0..3 (strides 4, 8, 16, 32) for a ViT grid of Hg x Wg patches."""
    return ((4 * Hg, 4 * Wg), (2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2))[level]
