"""The Mask2Former masked-attention transformer decoder on the HIP library: queries to class logits, masks and (CTVIS) re-identification
embeddings, from what ``MSDeformAttnPixelDecoder.forward_features`` returns.

Mirrors of the reference's ``MultiScaleMaskedTransformerDecoder``
(``downstream/OVIS/mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py``) and of its CTVIS subclass
``CLMultiScaleMaskedTransformerDecoder`` (``downstream/OVIS/ctvis/modeling/transformer_decoder/cl_mask2former_transformer_decoder.py``),
the ``TRANSFORMER_DECODER_NAME`` of every shipped OVIS config.  Both carry the reference's explicit-keyword constructor, parameter tree,
state-dict keys and order, and initialisation, so ``load_state_dict(strict=True)`` of the ``sem_seg_head.predictor.*`` slice of a
checkpoint works (the prefix is accepted and dropped, ``static_query`` is renamed to ``query_feat`` as the reference does).  The forward
runs in ``libstreamformer_hip.so`` (``sf_maskdec_forward``, kernels in ``csrc/sf_maskdec.hip``); there is no CPU fallback.

    pix = MSDeformAttnPixelDecoder(...).cuda().eval()
    dec = CLMultiScaleMaskedTransformerDecoder(256, num_classes=40, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048,
                                               dec_layers=9, pre_norm=False, mask_dim=256, enforce_input_project=False,
                                               reid_hidden_dim=256, num_reid_head_layers=3).cuda().eval()
    mask_features, _, multi_scale_features = pix.forward_features(pyramid)
    out = dec(multi_scale_features, mask_features)        # pred_logits, pred_masks, pred_embeds, pred_bboxes, ...

Training is an opt-in: ``trainable=True`` (constructor keyword or attribute) makes ``.train()`` run an autograd graph instead of the
refusal: torch ops on the module's own parameters, attention through ``MaskedAttentionFunction``, each layer's packed attention mask
from ``sf_op_maskdec_mask``, and the full-resolution mask logits of all ``dec_layers + 1`` heads through ``sf_op_masklogits_forward`` /
``sf_op_masklogits_backward`` (``csrc/sf_masklogits.hip``), with ONE gradient buffer for ``mask_features`` shared by the heads.  The
result feeds ``SetCriterion`` / ``ctvis_train_losses`` and ``.backward()``.  ``.eval()`` is the same native path either way.

Out of scope: the losses themselves (in eval ``aux_outputs`` is empty unless ``return_aux=True``), the CTVIS tracker and post-processing
(``ctvis_model.py``'s inference over ``pred_embeds``), ``StandardTransformerDecoder``, and padding masks (the reference deletes its
``mask`` argument itself; it is accepted and ignored here too).
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Any, Dict, List, Optional, Sequence

import torch
import torch.nn.functional as TF
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as nat
from .masked_attention import MaskedAttentionFunction, PackedAttentionMask
from .pixel_decoder import ConvNorm, _c2_xavier_fill, _staged_dtype

__all__ = ["MultiScaleMaskedTransformerDecoder", "CLMultiScaleMaskedTransformerDecoder"]

PREFIX = "sem_seg_head.predictor."
NUM_FEATURE_LEVELS = 3


def _xavier_matrices(module: nn.Module) -> None:
    for p in module.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)


class _SharedGrad:
    """The one gradient buffer of ``mask_features`` that the heads of a training forward add into."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None


class _MaskFeatureHub(Function):
    """Identity on ``mask_features``.  Every head reads the OUTPUT, so autograd runs this backward after the backward of every head;
    the heads add their gradients into ``shared.buf`` (``sf_op_masklogits_backward``, ``accumulate``) and return none of their own, and
    this hands the buffer back as the gradient of ``mask_features``: one full-size tensor instead of ``dec_layers + 1``."""

    @staticmethod
    def forward(ctx, mask_features, shared):
        ctx.shared = shared
        ctx.set_materialize_grads(False)
        return mask_features.view_as(mask_features)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        buf, ctx.shared.buf = ctx.shared.buf, None
        if grad is not None:                  # a reader of the hub's output that is not a head
            buf = grad if buf is None else buf + grad
        return buf, None


class _MaskLogitsFunction(Function):
    """``logits[f, q, h, w] = sum_c me[f, q, c] feat[f, c, h, w]`` on the HIP kernels; the gradient of ``feat`` goes to ``shared``."""

    @staticmethod
    def forward(ctx, me, feat, shared):
        Fr, Q, Dm = me.shape
        H, W = feat.shape[2:]
        me = me.contiguous()
        out = torch.empty(Fr, Q, H, W, device=me.device, dtype=torch.float32)
        nat.launch(me.device, nat.lib.sf_op_masklogits_forward, me.data_ptr(), feat.data_ptr(), out.data_ptr(), Fr, Q, Dm, H * W)
        ctx.save_for_backward(me, feat)
        ctx.shared = shared
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        me, feat = ctx.saved_tensors
        shared = ctx.shared
        Fr, Q, Dm = me.shape
        P = feat.shape[2] * feat.shape[3]
        grad = grad.float().contiguous()
        d_me = torch.empty_like(me) if ctx.needs_input_grad[0] else None
        d_feat, accumulate = None, 0
        if ctx.needs_input_grad[1]:
            accumulate = int(shared.buf is not None)
            if shared.buf is None:
                shared.buf = torch.empty_like(feat)
            d_feat = shared.buf
        if d_me is None and d_feat is None:
            return None, None, None
        ws = None
        if d_me is not None:
            ws = nat.scratch(nat.lib.sf_op_masklogits_backward_workspace_bytes(Fr, Q, Dm, P), me.device)
        nat.launch(me.device, nat.lib.sf_op_masklogits_backward, grad.data_ptr(), me.data_ptr(), feat.data_ptr(), nat.ptr(d_me), nat.ptr(d_feat),
                   accumulate, Fr, Q, Dm, P, workspace=ws)
        return d_me, None, None               # the hub returns the gradient of the features


class _Reach(Function):
    """Identity on ``out`` that gives ``others`` a zero gradient: with fewer than three layers a feature level is projected and never
    attended to, and its ``input_proj`` / ``x[l]`` would be left without a gradient (``None``) where a training loop expects zeros."""

    @staticmethod
    def forward(ctx, out, *others):
        ctx.meta = [(t.shape, t.dtype, t.device) for t in others]
        return out.view_as(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return (grad,) + tuple(torch.zeros(s, dtype=d, device=dev) for s, d, dev in ctx.meta)


def _sine_table(h: int, w: int, C: int, device) -> torch.Tensor:
    """PositionEmbeddingSine(C / 2, normalize=True) of an all-false mask as rows [h w, C], fp32 (computed in fp64, rounded once)."""
    wd = torch.float64
    npf = C // 2
    y = torch.arange(1, h + 1, dtype=wd, device=device)[:, None].expand(h, w)
    x = torch.arange(1, w + 1, dtype=wd, device=device)[None, :].expand(h, w)
    y = y / (y[-1:, :] + 1e-6) * (2 * math.pi)
    x = x / (x[:, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(npf, dtype=wd, device=device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / npf)
    px, py = x[:, :, None] / dim_t, y[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).reshape(h * w, C).float()


class _SelfAttentionLayer(nn.Module):
    """SelfAttentionLayer's parameters; ``nn.MultiheadAttention`` holds them and is never called."""

    def __init__(self, d_model: int, nhead: int):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=0.0)
        self.norm = nn.LayerNorm(d_model)
        _xavier_matrices(self)


class _CrossAttentionLayer(nn.Module):
    def __init__(self, d_model: int, nhead: int):
        super().__init__()
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=0.0)
        self.norm = nn.LayerNorm(d_model)
        _xavier_matrices(self)


class _FFNLayer(nn.Module):
    def __init__(self, d_model: int, dim_feedforward: int):
        super().__init__()
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)
        _xavier_matrices(self)


class _MLP(nn.Module):
    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int, num_layers: int):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))


class MultiScaleMaskedTransformerDecoder(nn.Module):
    _version = 2
    _reid_layers = -1                     # the base class has no reid_embed
    _reid_hidden_dim = 0

    def __init__(self, in_channels: int, mask_classification: bool = True, *, num_classes: int, hidden_dim: int, num_queries: int, nheads: int,
                 dim_feedforward: int, dec_layers: int, pre_norm: bool, mask_dim: int, enforce_input_project: bool,
                 compute_dtype: Any = "fp32", trainable: bool = False):
        super().__init__()
        self._compute = nat.compute_mode(compute_dtype)
        self.compute_dtype = compute_dtype
        self._trainable = False
        self.trainable = trainable
        self.in_channels, self.mask_classification, self.pre_norm = int(in_channels), bool(mask_classification), bool(pre_norm)
        self.num_classes, self.hidden_dim, self.num_queries, self.num_heads = int(num_classes), int(hidden_dim), int(num_queries), int(nheads)
        self.dim_feedforward, self.num_layers, self.mask_dim = int(dim_feedforward), int(dec_layers), int(mask_dim)
        self.enforce_input_project = bool(enforce_input_project)
        self.num_feature_levels = NUM_FEATURE_LEVELS
        try:                              # the library's own rules, before any weight exists: the message names the field
            nat.OwnedHandle.release(self._create(0, nat.OwnedHandle(nat.lib.sf_maskdec_destroy, "mask decoder probe")))
        except nat.NativeError as e:
            refused = NotImplementedError if ("pre_norm" in str(e) or "mask_classification" in str(e)) else ValueError
            raise refused(str(e)) from None
        self.transformer_self_attention_layers = nn.ModuleList(_SelfAttentionLayer(hidden_dim, nheads) for _ in range(self.num_layers))
        self.transformer_cross_attention_layers = nn.ModuleList(_CrossAttentionLayer(hidden_dim, nheads) for _ in range(self.num_layers))
        self.transformer_ffn_layers = nn.ModuleList(_FFNLayer(hidden_dim, dim_feedforward) for _ in range(self.num_layers))
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.query_feat = nn.Embedding(num_queries, hidden_dim)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.level_embed = nn.Embedding(self.num_feature_levels, hidden_dim)
        self.input_proj = nn.ModuleList()
        for _ in range(self.num_feature_levels):
            if in_channels != hidden_dim or enforce_input_project:
                self.input_proj.append(ConvNorm(in_channels, hidden_dim, 1))
                _c2_xavier_fill(self.input_proj[-1])
            else:
                self.input_proj.append(nn.Sequential())
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.mask_embed = _MLP(hidden_dim, hidden_dim, mask_dim, 3)
        self._native = nat.PackedHandle(self._create, nat.lib.sf_maskdec_load_tensor, self._finalize, nat.lib.sf_maskdec_destroy, "mask decoder",
                                        dtype_of=_staged_dtype)

    # ------------------------------------------------------------------------------------ weights
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            renamed = False
            for k in list(state_dict.keys()):
                if "static_query" not in k:
                    continue
                v = state_dict.pop(k)
                if v.shape[0] == self.num_queries:      # a query table of another size is dropped, as the reference drops it
                    state_dict[k.replace("static_query", "query_feat")] = v
                    renamed = True
            if renamed:
                logging.getLogger(__name__).warning("Weight format of %s have changed! Please upgrade your models. Applying automatic conversion now ...",
                                                    self.__class__.__name__)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Keys with or without the checkpoint's leading ``sem_seg_head.predictor.``; with ``strict=False`` the rest of a whole checkpoint
        is ignored."""
        own = set(self.state_dict())
        sd = {}
        for k, v in state_dict.items():
            k2 = k[len(PREFIX):] if k.startswith(PREFIX) else k
            if strict or k2 in own or "static_query" in k2:
                sd[k2] = v
        return super().load_state_dict(sd, strict=strict, assign=assign)

    # ------------------------------------------------------------------------------------ native handle
    def _create(self, device_index: int, h: Any = None):
        h = C.c_void_p() if h is None else h
        cfg = nat.SfMaskdecConfig(self.in_channels, self.hidden_dim, self.num_queries, self.num_heads, self.dim_feedforward, self.num_layers,
                                  self.mask_dim, self.num_classes, int(self.enforce_input_project), int(self.pre_norm),
                                  int(self.mask_classification), self._reid_layers, self._reid_hidden_dim)
        nat.check(nat.lib.sf_maskdec_create(C.byref(cfg), device_index, C.byref(h)))
        return h

    def _finalize(self, h) -> None:
        nat.check(nat.lib.sf_maskdec_finalize(h, self._compute))

    @property
    def device(self) -> torch.device:
        return self.query_feat.weight.device

    def _handle(self):
        """The native decoder, (re)packed when a parameter changed (in-place update, load_state_dict, .to(device))."""
        params = list(self.named_parameters())
        dev = self.device
        return self._native.get(dev, nat.weights_token(dev, [p for _, p in params]), params)

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

    def forward(self, x: Sequence[torch.Tensor], mask_features: torch.Tensor, mask: Optional[torch.Tensor] = None, *, return_aux: bool = False,
                return_attn_masks: bool = False) -> Dict[str, Any]:
        """``x``: three fp32 (F, in_channels, h_l, w_l) feature maps, ``mask_features``: fp32 (F, mask_dim, H, W), both on the GPU, as the
        pixel decoder returns them.  Returns the reference's dict; ``aux_outputs`` is an empty list unless ``return_aux`` (the per-layer
        predictions are a training need).  ``return_attn_masks`` adds ``attn_masks``: per layer the bit-packed attention mask, int32
        (F, Q, ceil(h w / 32)), bit ``j & 31`` of word ``j // 32`` set where key ``j`` is hidden.

        In ``.train()`` with ``trainable=True`` the result is differentiable and ``aux_outputs`` is always populated."""
        del mask                          # the reference disables it too
        if self.training and not self._trainable:
            raise RuntimeError("the native mask decoder is inference only: call .eval() (training and the losses are not part of it)")
        if self.training:
            return self._forward_train(*self._checked(x, mask_features), return_attn_masks)
        with torch.no_grad():
            return self._forward_eval(*self._checked(x, mask_features), return_aux, return_attn_masks)

    # ------------------------------------------------------------------------------------ training forward
    def _attend(self, mha: nn.MultiheadAttention, q_in, k_in, v_in, mask: Optional[PackedAttentionMask]):
        """nn.MultiheadAttention's arithmetic on ``mha``'s own parameters, [F, T, C] tensors, the attention itself on the HIP kernels."""
        Cd = self.hidden_dim
        w, b = mha.in_proj_weight, mha.in_proj_bias
        if q_in is k_in:                  # self-attention: q and k from one [F, T, 2 C] product, read in place by the kernel
            qk = TF.linear(q_in, w[:2 * Cd], b[:2 * Cd])
            q, k = qk[..., :Cd], qk[..., Cd:]
        else:
            q, k = TF.linear(q_in, w[:Cd], b[:Cd]), TF.linear(k_in, w[Cd:2 * Cd], b[Cd:2 * Cd])
        v = TF.linear(v_in, w[2 * Cd:], b[2 * Cd:])
        ctx = MaskedAttentionFunction.apply(q, k, v, mask, self.num_heads)
        return TF.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)

    def _forward_train(self, xs, mf, return_attn_masks: bool) -> Dict[str, Any]:
        dev = self.device
        F, Dm, H, W = mf.shape
        Q, Cd, L = self.num_queries, self.hidden_dim, self.num_layers
        cl = self._reid_layers >= 0
        shared = _SharedGrad()
        feat = _MaskFeatureHub.apply(mf, shared)
        mf_plain = mf.detach()
        src, pos, sizes = [], [], []
        for l, t in enumerate(xs):
            h, w = t.shape[2:]
            sizes.append((h, w))
            rows = t.flatten(2).transpose(1, 2)
            proj = self.input_proj[l]
            if isinstance(proj, ConvNorm):
                rows = TF.linear(rows, proj.weight.flatten(1), proj.bias)
            src.append(rows + self.level_embed.weight[l])
            pos.append(_sine_table(h, w, Cd, dev))
        qe = self.query_embed.weight.unsqueeze(0).expand(F, -1, -1)
        out = self.query_feat.weight.unsqueeze(0).expand(F, -1, -1)
        if L < self.num_feature_levels:   # levels no layer attends to: zero gradients, not None
            out = _Reach.apply(out, *src[L:])

        def mlp(m: _MLP, v):
            for j, layer in enumerate(m.layers):
                v = layer(v)
                if j < m.num_layers - 1:
                    v = torch.relu(v)
            return v

        def heads_of(out, size):
            """The prediction heads on decoder_norm(out), and the packed attention mask the next layer attends under (``size`` or None)."""
            dn = self.decoder_norm(out)
            pred = {"pred_logits": self.class_embed(dn)}
            me = mlp(self.mask_embed, dn).contiguous()
            pred["pred_masks"] = _MaskLogitsFunction.apply(me, feat, shared)
            if cl:
                pred["pred_queries"] = dn
                pred["pred_embeds"] = mlp(self.reid_embed, dn) if isinstance(self.reid_embed, _MLP) else self.reid_embed(dn)
            bits = None
            if size is not None:
                h, w = size
                bits = torch.empty(F, Q, (h * w + 31) // 32, dtype=torch.int32, device=dev)
                ws = self._native.workspace(nat.lib.sf_op_maskdec_mask_workspace_bytes(F, Dm, h, w), dev, key="train mask")
                nat.launch(dev, nat.lib.sf_op_maskdec_mask, me.detach().data_ptr(), mf_plain.data_ptr(), F, Q, Dm, H, W, h, w, bits.data_ptr(), None, None,
                           workspace=ws)
            return pred, bits

        preds, masks = [], []
        pred, bits = heads_of(out, sizes[0] if L else None)
        preds.append(pred)
        for i in range(L):
            l = i % self.num_feature_levels
            masks.append(bits)
            ca, sa, ffn = self.transformer_cross_attention_layers[i], self.transformer_self_attention_layers[i], self.transformer_ffn_layers[i]
            out = ca.norm(out + self._attend(ca.multihead_attn, out + qe, src[l] + pos[l], src[l], PackedAttentionMask(bits, sizes[l][0] * sizes[l][1])))
            x_pos = out + qe
            out = sa.norm(out + self._attend(sa.self_attn, x_pos, x_pos, out, None))
            out = ffn.norm(out + ffn.linear2(torch.relu(ffn.linear1(out))))
            pred, bits = heads_of(out, sizes[(i + 1) % self.num_feature_levels] if i + 1 < L else None)
            preds.append(pred)
        res: Dict[str, Any] = dict(preds[-1])
        if cl:
            boxes = torch.empty(F, Q, 4, dtype=torch.float32, device=dev)
            nat.launch(dev, nat.lib.sf_op_maskdec_boxes, res["pred_masks"].detach().data_ptr(), boxes.data_ptr(), F * Q, H, W)
            res.update(pred_bboxes=boxes, query_pos_embeds=self.query_embed.weight.detach().unsqueeze(0).repeat(F, 1, 1))
        res["aux_outputs"] = preds[:-1]
        if return_attn_masks:
            res["attn_masks"] = masks
        return res

    def _checked(self, x, mask_features):
        if len(x) != self.num_feature_levels:
            raise ValueError(f"x must hold {self.num_feature_levels} feature maps, got {len(x)}")
        dev = self.device
        if dev.type != "cuda" or mask_features.device.type != "cuda" or any(t.device.type != "cuda" for t in x):
            raise RuntimeError("the mask decoder runs on the MI355X: move the module and its inputs with .to('cuda') (there is no CPU fallback)")
        if mask_features.dim() != 4 or mask_features.shape[1] != self.mask_dim:
            raise ValueError(f"mask_features must be (F, {self.mask_dim}, H, W), got {tuple(mask_features.shape)}")
        F, _, H, W = mask_features.shape
        xs = []
        for i, t in enumerate(x):
            if t.dim() != 4 or t.shape[0] != F or t.shape[1] != self.in_channels:
                raise ValueError(f"x[{i}] must be ({F}, {self.in_channels}, h, w), got {tuple(t.shape)}")
            xs.append(t.to(device=dev, dtype=torch.float32).contiguous())
        return xs, mask_features.to(device=dev, dtype=torch.float32).contiguous()

    def _forward_eval(self, xs, mf, return_aux: bool, return_attn_masks: bool) -> Dict[str, Any]:
        dev = self.device
        F, _, H, W = mf.shape
        h = self._handle()
        Q, Cd, L, K1 = self.num_queries, self.hidden_dim, self.num_layers, self.num_classes + 1
        cl = self._reid_layers >= 0
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)      # noqa: E731
        out = nat.SfMaskdecOutputs()
        t: Dict[str, torch.Tensor] = {"pred_logits": new(F, Q, K1), "pred_masks": new(F, Q, H, W)}
        if cl:
            t.update(pred_queries=new(F, Q, Cd), pred_embeds=new(F, Q, Cd), pred_bboxes=new(F, Q, 4))
        if return_aux and L:
            t.update(aux_logits=new(L, F, Q, K1), aux_masks=new(L, F, Q, H, W))
            if cl:
                t.update(aux_queries=new(L, F, Q, Cd), aux_embeds=new(L, F, Q, Cd))
        words = [(xs[i % 3].shape[2] * xs[i % 3].shape[3] + 31) // 32 for i in range(L)]
        if return_attn_masks and L:
            t["attn_masks"] = torch.empty(F * Q * sum(words), dtype=torch.int32, device=dev)
        for k, v in t.items():
            setattr(out, k, v.data_ptr())
        shapes = nat.i32_array([d for v in xs for d in v.shape[2:]])
        ws = self._native.workspace(nat.sized(nat.lib.sf_maskdec_workspace_bytes, h, F, shapes, H, W), dev)
        nat.launch(dev, nat.lib.sf_maskdec_forward, h, nat.ptr_array(xs), mf.data_ptr(), F, shapes, H, W, C.byref(out), workspace=ws)
        res: Dict[str, Any] = {"pred_logits": t["pred_logits"], "pred_masks": t["pred_masks"]}
        if cl:
            res.update(pred_queries=t["pred_queries"], pred_embeds=t["pred_embeds"], pred_bboxes=t["pred_bboxes"],
                       query_pos_embeds=self.query_embed.weight.detach().unsqueeze(0).repeat(F, 1, 1))
        aux: List[Dict[str, torch.Tensor]] = []
        if return_aux:
            for i in range(L):
                e = {"pred_logits": t["aux_logits"][i], "pred_masks": t["aux_masks"][i]}
                if cl:
                    e.update(pred_queries=t["aux_queries"][i], pred_embeds=t["aux_embeds"][i])
                aux.append(e)
        res["aux_outputs"] = aux
        if return_attn_masks:
            res["attn_masks"], off = [], 0
            for wd in words:
                res["attn_masks"].append(t["attn_masks"][off:off + F * Q * wd].view(F, Q, wd))
                off += F * Q * wd
        return res


class CLMultiScaleMaskedTransformerDecoder(MultiScaleMaskedTransformerDecoder):
    """The CTVIS decoder: the same layers plus ``reid_embed`` (``pred_embeds``), ``pred_queries``, ``pred_bboxes`` and
    ``query_pos_embeds``."""

    def __init__(self, in_channels: int, mask_classification: bool = True, *, num_classes: int, hidden_dim: int, num_queries: int, nheads: int,
                 dim_feedforward: int, dec_layers: int, pre_norm: bool, mask_dim: int, enforce_input_project: bool, reid_hidden_dim: int,
                 num_reid_head_layers: int, compute_dtype: Any = "fp32", trainable: bool = False, **kwargs):
        self._reid_layers = max(int(num_reid_head_layers), 0)
        self._reid_hidden_dim = int(reid_hidden_dim)
        super().__init__(in_channels, mask_classification, num_classes=num_classes, hidden_dim=hidden_dim, num_queries=num_queries, nheads=nheads,
                         dim_feedforward=dim_feedforward, dec_layers=dec_layers, pre_norm=pre_norm, mask_dim=mask_dim,
                         enforce_input_project=enforce_input_project, compute_dtype=compute_dtype, trainable=trainable)
        if num_reid_head_layers > 0:
            self.reid_embed = _MLP(hidden_dim, reid_hidden_dim, hidden_dim, num_reid_head_layers)
            for layer in self.reid_embed.layers:
                _c2_xavier_fill(layer)
        else:
            self.reid_embed = nn.Identity()
