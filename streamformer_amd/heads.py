"""Loss heads of the multitask pre-training step (BASELINE config #3), on the HIP library.

Mirrors ``TimesformerVideoRetrievalHead.forward`` + ``SigLipLoss._loss`` (reference
``models/modeling_timesformer_siglip.py:2324-2351, 221-237``) and the training branch of
``TimesformerUniversalLocalizationHead.forward`` (``:2238-2282``).  Each head owns its
``logit_scale = log 10`` / ``logit_bias = -2`` pair (``:1363-1364, 2204-2205, 2300-2301``).
Text features come from a frozen SigLIP text tower in the reference; here they are inputs.
The caption-driven heads sit on the same conventions: ``GroundingHead`` (``TimesformerTemporalGroundingHead.forward``,
``:2373-2397``) and ``DenseTextLogits`` (evaluation output of the referring segmentation head, ``:2004-2018``).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _native as nat


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _scalar_on(dev: torch.device, v) -> torch.Tensor:
    """A head parameter as a 1-element fp32 DEVICE tensor (the kernels read it from HBM: no ``.item()``)."""
    if torch.is_tensor(v):
        return v.detach().to(dev, torch.float32).reshape(1)
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def _workspace(dev: torch.device, B: int, T: int) -> torch.Tensor:
    return nat.scratch(nat.lib.sf_loss_workspace_bytes(B, T), dev)


class RetrievalHead:
    """``logit_scale`` / ``logit_bias`` may be Python floats or (views of) device tensors — the trainer passes views
    into its flat parameter buffer, so the loss always sees the current values without a host copy."""

    def __init__(self, logit_scale=math.log(10.0), logit_bias=-2.0):
        self.logit_scale = logit_scale
        self.logit_bias = logit_bias

    def loss(self, pooler_output: torch.Tensor, text_features: torch.Tensor, rank: int = 0,
             need_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """pooler_output [B,T,D] (cuda), text_features [W*B, D]: all ranks' caption features, this rank's
        block at rows rank*B.. (the ring exchange of modeling:244-295 delivers exactly these negatives).
        Returns (loss [1], d loss/d pooler [B,T,D], d loss/d (logit_scale, logit_bias) [2])."""
        p, t = _f32(pooler_output), _f32(text_features.to(pooler_output.device))
        B, T, D = p.shape
        Bt = t.shape[0]
        if t.dim() != 2 or t.shape[1] != D:
            raise ValueError(f"text_features must be [rows, {D}], got {tuple(t.shape)}")
        if (rank + 1) * B > Bt:
            raise ValueError(f"rank {rank} with {B} clips needs text rows {rank * B}..{(rank + 1) * B - 1}, the table has {Bt}")
        dev = p.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gp = torch.empty_like(p) if need_grad else None
        gs = torch.empty(2, dtype=torch.float32, device=dev) if need_grad else None
        ls, lb, ws = _scalar_on(dev, self.logit_scale), _scalar_on(dev, self.logit_bias), _workspace(dev, B, T)
        nat.launch(dev, nat.lib.sf_retrieval_loss, p.data_ptr(), t.data_ptr(), B, T, D, Bt, rank * B, ls.data_ptr(), lb.data_ptr(), loss.data_ptr(),
                   nat.ptr(gp), nat.ptr(gs), workspace=ws)
        return loss, gp, gs


class LocalizationHead:
    def __init__(self, label_embeddings: torch.Tensor, logit_scale=math.log(10.0), logit_bias=-2.0):
        self.label_embeddings = label_embeddings     # [L, D], unit-norm means of prompt embeddings (:2211-2223)
        self.logit_scale = logit_scale
        self.logit_bias = logit_bias

    def loss(self, pooler_output: torch.Tensor, labels: torch.Tensor, need_grad: bool = True):
        p = _f32(pooler_output)
        dev = p.device
        e = _f32(self.label_embeddings.to(dev))
        lab = labels.to(dev, torch.int32).contiguous()
        B, T, D = p.shape
        if tuple(lab.shape) != (B, T):
            raise ValueError(f"labels must be [{B}, {T}], got {tuple(lab.shape)}")
        if e.shape[0] > 4096:
            raise ValueError(f"{e.shape[0]} label classes: the localization kernel holds at most 4096 per frame row")
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gp = torch.empty_like(p) if need_grad else None
        gs = torch.empty(2, dtype=torch.float32, device=dev) if need_grad else None
        ls, lb, ws = _scalar_on(dev, self.logit_scale), _scalar_on(dev, self.logit_bias), _workspace(dev, B, T)
        nat.launch(dev, nat.lib.sf_localization_loss, p.data_ptr(), e.data_ptr(), lab.data_ptr(), B, T, D, e.shape[0], ls.data_ptr(), lb.data_ptr(),
                   loss.data_ptr(), nat.ptr(gp), nat.ptr(gs), workspace=ws)
        return loss, gp, gs


class MaskLossHead:
    """Fused bilinear upsample + per-pixel cross-entropy of the video instance segmentation head (``sf_mask_loss``; reference
    ``models/modeling_timesformer_siglip.py:1829-1916``, training branch).  Thin: it groups nothing and selects nothing — the
    per-clip label tables (already sub-sampled / normalised where the reference does so) and integer masks at their training
    resolution come from the caller (``multitask.TimesformerUniversalVideoInstanceSegmentationHead``)."""

    def __init__(self, logit_scale=math.log(10.0), logit_bias=-2.0):
        self.logit_scale = logit_scale
        self.logit_bias = logit_bias

    def loss(self, dense_embeds: torch.Tensor, label_tables, mask_targets, need_grad: bool = True):
        """dense_embeds [B,T,N,D] (cuda); label_tables[i] [L_i, D]; mask_targets[i] int [T, H, W_i], -1 = ignore (every clip the
        same H).  Returns (loss [1], d loss / d dense_embeds [B,T,N,D], d loss / d (logit_scale, logit_bias) [2])."""
        x = _f32(dense_embeds)
        dev = x.device
        B, T, N, D = x.shape
        if len(label_tables) != B or len(mask_targets) != B:
            raise ValueError(f"{B} clips need {B} label tables and masks, got {len(label_tables)} and {len(mask_targets)}")
        tabs = [_f32(t.to(dev)) for t in label_tables]
        masks = [m.to(dev, torch.int32).contiguous() for m in mask_targets]
        H = int(masks[0].shape[1])
        for i, (t, m) in enumerate(zip(tabs, masks)):
            if t.dim() != 2 or t.shape[1] != D:
                raise ValueError(f"clip {i}: label table must be [L, {D}], got {tuple(t.shape)}")
            if m.dim() != 3 or m.shape[0] != T or m.shape[1] != H:
                raise ValueError(f"clip {i}: mask must be [{T}, {H}, W], got {tuple(m.shape)}")
        nl, wd = nat.i32_array([t.shape[0] for t in tabs]), nat.i32_array([m.shape[2] for m in masks])
        tp, mp = nat.ptr_array(tabs), nat.ptr_array(masks)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gx = torch.empty_like(x) if need_grad else None
        gs = torch.empty(2, dtype=torch.float32, device=dev) if need_grad else None
        ls, lb = _scalar_on(dev, self.logit_scale), _scalar_on(dev, self.logit_bias)
        nat.launch(dev, nat.lib.sf_mask_loss, x.data_ptr(), B, T, N, D, tp, nl, mp, wd, H, ls.data_ptr(), lb.data_ptr(), loss.data_ptr(), nat.ptr(gx),
                   nat.ptr(gs), workspace=nat.scratch(nat.lib.sf_mask_loss_workspace_bytes(B, T, N, max(1, max(nl))), dev))
        return loss, gx, gs


class DenseHeadProjection:
    """``_dense_feature_projection`` of the segmentation head (reference modeling:1786-1795) on all token rows, forward and backward
    on the library's training GEMMs (``sf_dense_head_forward`` / ``sf_dense_head_backward``: bf16 operands, fp32 accumulation).
    ``params``: the ten fp32 tensors in the order w_v.weight, w_v.bias, v_proj.weight, v_proj.bias, head_layernorm.weight,
    head_layernorm.bias, head_mlp.fc1.weight, fc1.bias, head_mlp.fc2.weight, fc2.bias.
    The workspace (the forward's saved activations + scratch, ~1 GB at 8 clips) is held from ``forward`` to the ``backward`` that
    consumes it and then handed back to torch's allocator: between steps, and while other tasks run, the object holds nothing."""

    def __init__(self, eps: float = 1e-6):
        self.eps = float(eps)
        self._ws = None
        self._shape = None
        self._params = None

    def release(self) -> None:
        """Drop the saved forward (workspace and parameter copies)."""
        self._ws = self._shape = self._params = None

    def forward(self, x: torch.Tensor, params) -> torch.Tensor:
        x = _f32(x)
        dev = x.device
        D = x.shape[-1]
        M = x.numel() // D
        ps = [_f32(p.detach().to(dev)) for p in params]
        if len(ps) != 10:
            raise ValueError(f"the dense projection has 10 parameter tensors, got {len(ps)}")
        inter = int(ps[6].shape[0])
        nbytes = nat.lib.sf_dense_head_workspace_bytes(M, D, inter)
        self.release()
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty_like(x)
        nat.launch(dev, nat.lib.sf_dense_head_forward, x.data_ptr(), M, D, inter, self.eps, nat.ptr_array(ps), out.data_ptr(), workspace=self._ws)
        self._shape = (M, D, inter)
        self._params = ps
        return out

    def backward(self, d_out: torch.Tensor):
        """Gradients of the forward that ran last on this object: (d x, [ten parameter gradients]).  Consumes the saved forward."""
        if self._shape is None:
            raise RuntimeError("DenseHeadProjection.backward needs a forward on the same object first")
        M, D, inter = self._shape
        g = _f32(d_out)
        dev = g.device
        ps = self._params
        dx = torch.empty_like(g)
        grads = [torch.empty_like(p) for p in ps]
        nat.launch(dev, nat.lib.sf_dense_head_backward, g.data_ptr(), M, D, inter, self.eps, nat.ptr_array(ps), dx.data_ptr(), nat.ptr_array(grads),
                   workspace=self._ws)
        self.release()         # stream-ordered: torch's allocator reuses the block only behind the launches above
        return dx, grads


class GroundingHead:
    """Temporal grounding (``sf_grounding_loss``; reference ``TimesformerTemporalGroundingHead.forward``, ``:2373-2397``): ONE caption
    per clip against every frame's pooled vector, ``-sum logsigmoid(y * logits) / B`` with ``y = -1`` where the label is 0 and the
    label itself elsewhere (the reference's ``masked_fill``; the rule is applied by the kernel on fp32 labels, no host check)."""

    def __init__(self, logit_scale=math.log(10.0), logit_bias=-2.0):
        self.logit_scale = logit_scale
        self.logit_bias = logit_bias

    def loss(self, pooler_output: torch.Tensor, text_features: torch.Tensor, labels: torch.Tensor, need_grad: bool = True,
             return_logits: bool = False):
        """pooler_output [B,T,D] (cuda), text_features [B,D] (this rank's captions: the reference gathers nothing for this head),
        labels [B,T] numbers.  Returns (loss [1], d loss/d pooler [B,T,D], d loss/d (logit_scale, logit_bias) [2]), followed by the
        logits [B,T] when ``return_logits``."""
        p = _f32(pooler_output)
        dev = p.device
        if p.dim() != 3:
            raise ValueError(f"pooler_output must be [B, T, D], got {tuple(p.shape)}")
        B, T, D = p.shape
        t = _f32(text_features.to(dev))
        if tuple(t.shape) != (B, D):
            raise ValueError(f"text_features must be [{B}, {D}] (one caption per clip), got {tuple(t.shape)}")
        if tuple(labels.shape) != (B, T):
            raise ValueError(f"labels must be [{B}, {T}], got {tuple(labels.shape)}")
        lab = _f32(labels.to(dev))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        gp = torch.empty_like(p) if need_grad else None
        gs = torch.empty(2, dtype=torch.float32, device=dev) if need_grad else None
        logits = torch.empty(B, T, dtype=torch.float32, device=dev) if return_logits else None
        ls, lb, ws = _scalar_on(dev, self.logit_scale), _scalar_on(dev, self.logit_bias), _workspace(dev, B, T)
        nat.launch(dev, nat.lib.sf_grounding_loss, p.data_ptr(), t.data_ptr(), lab.data_ptr(), B, T, D, ls.data_ptr(), lb.data_ptr(), loss.data_ptr(),
                   nat.ptr(gp), nat.ptr(gs), nat.ptr(logits), workspace=ws)
        return (loss, gp, gs, logits) if return_logits else (loss, gp, gs)

    def logits(self, pooler_output: torch.Tensor, text_features: torch.Tensor) -> torch.Tensor:
        """The logits [B,T] alone (labels play no part in them)."""
        B, T = pooler_output.shape[:2]
        return self.loss(pooler_output, text_features, torch.zeros(B, T, device=pooler_output.device), need_grad=False, return_logits=True)[3]


class DenseTextLogits:
    """Dense caption-to-patch logits of the referring segmentation head's evaluation branch (``sf_dense_text_logits``; reference
    ``:2004-2018``): ``exp(logit_scale) * <x / |x|, text_j / |text_j|> + logit_bias`` for every row of ``x``, fp32 throughout."""
    MAX_CAPTIONS = 64

    def __init__(self, logit_scale=math.log(10.0), logit_bias=-2.0):
        self.logit_scale = logit_scale
        self.logit_bias = logit_bias

    def forward(self, x: torch.Tensor, text_features: torch.Tensor) -> torch.Tensor:
        """x [..., D] (cuda), text_features [n, D] (un-normalised) -> [..., n]."""
        x = _f32(x)
        dev = x.device
        D = x.shape[-1]
        t = _f32(text_features.to(dev))
        if t.dim() != 2 or t.shape[1] != D:
            raise ValueError(f"text_features must be [n, {D}], got {tuple(t.shape)}")
        n = int(t.shape[0])
        if n > self.MAX_CAPTIONS:
            raise ValueError(f"{n} captions: the dense text logits kernel takes at most {self.MAX_CAPTIONS} per call")
        if x.data_ptr() % 16:
            x = x.clone()
        M = x.numel() // D
        out = torch.empty(tuple(x.shape[:-1]) + (n,), dtype=torch.float32, device=dev)
        ls, lb = _scalar_on(dev, self.logit_scale), _scalar_on(dev, self.logit_bias)
        nat.launch(dev, nat.lib.sf_dense_text_logits, x.data_ptr(), t.data_ptr(), M, D, n, ls.data_ptr(), lb.data_ptr(), out.data_ptr())
        return out
