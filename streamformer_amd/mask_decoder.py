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

Out of scope: training and the losses (``aux_outputs`` is empty unless ``return_aux=True``), the CTVIS tracker and post-processing
(``ctvis_model.py``'s inference over ``pred_embeds``), ``StandardTransformerDecoder``, and padding masks (the reference deletes its
``mask`` argument itself; it is accepted and ignored here too).
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _native as nat
from .pixel_decoder import ConvNorm, _c2_xavier_fill, _staged_dtype

__all__ = ["MultiScaleMaskedTransformerDecoder", "CLMultiScaleMaskedTransformerDecoder"]

PREFIX = "sem_seg_head.predictor."
NUM_FEATURE_LEVELS = 3


def _xavier_matrices(module: nn.Module) -> None:
    for p in module.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)


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
                 compute_dtype: Any = "fp32"):
        super().__init__()
        self._compute = nat.compute_mode(compute_dtype)
        self.compute_dtype = compute_dtype
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
    @torch.no_grad()
    def forward(self, x: Sequence[torch.Tensor], mask_features: torch.Tensor, mask: Optional[torch.Tensor] = None, *, return_aux: bool = False,
                return_attn_masks: bool = False) -> Dict[str, Any]:
        """``x``: three fp32 (F, in_channels, h_l, w_l) feature maps, ``mask_features``: fp32 (F, mask_dim, H, W), both on the GPU, as the
        pixel decoder returns them.  Returns the reference's dict; ``aux_outputs`` is an empty list unless ``return_aux`` (the per-layer
        predictions are a training need).  ``return_attn_masks`` adds ``attn_masks``: per layer the bit-packed attention mask, int32
        (F, Q, ceil(h w / 32)), bit ``j & 31`` of word ``j // 32`` set where key ``j`` is hidden."""
        del mask                          # the reference disables it too
        if self.training:
            raise RuntimeError("the native mask decoder is inference only: call .eval() (training and the losses are not part of it)")
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
        mf = mask_features.to(device=dev, dtype=torch.float32).contiguous()
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
        shapes = (C.c_int32 * 6)(*[d for v in xs for d in v.shape[2:]])
        nbytes = C.c_size_t()
        nat.check(nat.lib.sf_maskdec_workspace_bytes(h, F, shapes, H, W, C.byref(nbytes)))
        ws = self._native.workspace(nbytes.value, dev)
        ptrs = (C.c_void_p * 3)(*[v.data_ptr() for v in xs])
        with torch.cuda.device(dev):
            nat.check(nat.lib.sf_maskdec_forward(h, ptrs, mf.data_ptr(), F, shapes, H, W, C.byref(out), ws.data_ptr(), ws.numel(),
                                                 nat.current_stream_handle(dev)))
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
                 num_reid_head_layers: int, compute_dtype: Any = "fp32", **kwargs):
        self._reid_layers = max(int(num_reid_head_layers), 0)
        self._reid_hidden_dim = int(reid_hidden_dim)
        super().__init__(in_channels, mask_classification, num_classes=num_classes, hidden_dim=hidden_dim, num_queries=num_queries, nheads=nheads,
                         dim_feedforward=dim_feedforward, dec_layers=dec_layers, pre_norm=pre_norm, mask_dim=mask_dim,
                         enforce_input_project=enforce_input_project, compute_dtype=compute_dtype)
        if num_reid_head_layers > 0:
            self.reid_embed = _MLP(hidden_dim, reid_hidden_dim, hidden_dim, num_reid_head_layers)
            for layer in self.reid_embed.layers:
                _c2_xavier_fill(layer)
        else:
            self.reid_embed = nn.Identity()
