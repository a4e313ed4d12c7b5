"""Masked multi-head attention with a native backward on the MI355X: the operator, its autograd function and a drop-in module for
``nn.MultiheadAttention`` as the reference's Mask2Former / CTVIS decoder layers call it (``CrossAttentionLayer`` /
``SelfAttentionLayer`` of mask2former_transformer_decoder.py: sequence-first tensors, a boolean ``attn_mask``, ``need_weights`` unused).

torch turns the boolean ``[F * heads, Q, HW]`` mask into an additive float mask and keeps the ``[F * heads, Q, HW]`` probabilities for
the backward.  Here the mask is bit-packed (``PackedAttentionMask``; 32 keys a word, shared by the heads unless they differ), the
forward (``csrc/sf_maskdec.hip``, the inference decoder's own kernel) keeps one log-sum-exp per row, and the backward
(``csrc/sf_maskattn.hip``) recomputes the probabilities from it; key tiles hidden from a whole query tile are skipped in both.

    from streamformer_amd import use_native_attention
    use_native_attention(torch_decoder)        # every compatible nn.MultiheadAttention now runs (and trains) on the HIP kernels

Everything is fp32; kernels run on torch's current stream.  There is no CPU fallback.  One documented difference: a query whose keys are
all hidden gets zeros (and zero gradients) where torch gives NaN; the reference clears such rows before the call.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.init import constant_, xavier_uniform_

from . import _native as nat

__all__ = ["PackedAttentionMask", "pack_attention_mask", "MaskedAttentionFunction", "masked_attention", "MaskedMultiheadAttention",
           "use_native_attention"]


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the MI355X: move the tensors with .to('cuda') (there is no CPU fallback)")


class PackedAttentionMask:
    """A boolean attention mask as the kernels read it: ``words`` int32 ``[F, Q, ceil(HW / 32)]`` (shared by the heads) or
    ``[F, heads, Q, ceil(HW / 32)]`` (``per_head``), bit ``j & 31`` of word ``j // 32`` set = key ``j`` hidden.  This is the layout of
    the native decoder's own masks (``sf_op_maskdec_mask``)."""

    def __init__(self, words: torch.Tensor, HW: int, per_head: bool = False):
        if words.dtype != torch.int32 or words.dim() != (4 if per_head else 3) or words.shape[-1] != (HW + 31) // 32:
            raise ValueError(f"words must be int32 [F, {'heads, ' if per_head else ''}Q, {(HW + 31) // 32}] for HW = {HW}, got "
                             f"{words.dtype} {tuple(words.shape)}")
        self.words, self.HW, self.per_head = words.contiguous(), int(HW), bool(per_head)

    @property
    def frames(self) -> int:
        return self.words.shape[0]

    @property
    def queries(self) -> int:
        return self.words.shape[-2]

    @property
    def heads(self) -> Optional[int]:
        return self.words.shape[1] if self.per_head else None


def pack_attention_mask(mask_bool: torch.Tensor, heads: Optional[int] = None) -> PackedAttentionMask:
    """bool ``[F, Q, HW]`` (True = hidden; shared by the heads), or ``[F * heads, Q, HW]`` with ``heads`` given (head-minor, as torch
    orders it; kept per head), or ``[F, heads, Q, HW]`` -> ``PackedAttentionMask``.  The padding bits of the last word are set."""
    if not isinstance(mask_bool, torch.Tensor) or mask_bool.dtype != torch.bool:
        raise TypeError("float masks are not supported: the attention mask must be a bool tensor (True = hidden), got "
                        f"{getattr(mask_bool, 'dtype', type(mask_bool))}")
    _need_gpu(mask_bool, "pack_attention_mask")
    if mask_bool.dim() == 3 and heads:
        if mask_bool.shape[0] % heads:
            raise ValueError(f"mask {tuple(mask_bool.shape)}: the first dimension is not a multiple of heads = {heads}")
        mask_bool = mask_bool.reshape(mask_bool.shape[0] // heads, heads, *mask_bool.shape[1:])
    if mask_bool.dim() not in (3, 4) or 0 in mask_bool.shape:
        raise ValueError(f"mask must be a non-empty bool [F, Q, HW], [F * heads, Q, HW] or [F, heads, Q, HW], got {tuple(mask_bool.shape)}")
    m = mask_bool.contiguous()
    HW = m.shape[-1]
    words = torch.empty(*m.shape[:-1], (HW + 31) // 32, device=m.device, dtype=torch.int32)
    nat.launch(m.device, nat.lib.sf_op_maskattn_pack, m.data_ptr(), words.data_ptr(), m.numel() // HW, HW)
    return PackedAttentionMask(words, HW, per_head=m.dim() == 4)


def _rows(t: torch.Tensor, name: str) -> Tuple[torch.Tensor, int]:
    """[F, T, C] fp32 -> (a tensor the kernels can read in place, its row pitch): a column range of a wider row-major buffer stays one."""
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    Fr, T, C = t.shape
    if t.stride(2) == 1 and t.stride(1) >= C and t.stride(1) % 4 == 0 and (Fr == 1 or t.stride(0) == T * t.stride(1)) and t.data_ptr() % 16 == 0:
        return t, t.stride(1)
    return t.contiguous(), C


def _check(q, k, v, mask: Optional[PackedAttentionMask], heads: int):
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError("q [F, Tq, C], k and v [F, Tk, C]")
    Fr, Tq, C = q.shape
    Tk = k.shape[1]
    if tuple(k.shape) != (Fr, Tk, C) or tuple(v.shape) != (Fr, Tk, C):
        raise ValueError(f"inconsistent shapes: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    if heads < 1 or C % heads or (C // heads) % 8 or not 8 <= C // heads <= 128:
        raise ValueError(f"the head width C / heads = {C} / {heads} must be a multiple of 8 in 8..128")
    if mask is not None:
        if not isinstance(mask, PackedAttentionMask):
            raise TypeError("mask must be a PackedAttentionMask (pack_attention_mask) or None")
        if mask.frames != Fr or mask.queries != Tq or mask.HW != Tk or (mask.per_head and mask.heads != heads):
            raise ValueError(f"the mask is for F = {mask.frames}, Q = {mask.queries}, HW = {mask.HW}, heads = {mask.heads}; the tensors have "
                             f"F = {Fr}, Q = {Tq}, HW = {Tk}, heads = {heads}")
        if mask.words.device != q.device:
            raise ValueError("the mask is on another device")
    return Fr, Tq, Tk, C


class MaskedAttentionFunction(Function):
    """``ctx = softmax(q k^T / sqrt(hd) | mask) v`` per head on ``[F, T, C]`` tensors, differentiable in q, k and v."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads):
        _need_gpu(q, "masked attention")
        Fr, Tq, Tk, C = _check(q, k, v, mask, heads)
        (q, qp), (k, kp), (v, vp) = _rows(q, "q"), _rows(k, "k"), _rows(v, "v")
        if kp != vp:
            k, v, kp = k.contiguous(), v.contiguous(), C
        out = torch.empty(Fr, Tq, C, device=q.device, dtype=torch.float32)
        stats = torch.empty(Fr, heads, Tq, device=q.device, dtype=torch.float32)
        nat.launch(q.device, nat.lib.sf_op_maskattn_forward, q.data_ptr(), qp, k.data_ptr(), v.data_ptr(), kp,
                   nat.ptr(mask.words if mask is not None else None), int(mask is not None and mask.per_head), out.data_ptr(), stats.data_ptr(),
                   Fr, Tq, Tk, heads, C // heads, 0)
        ctx.save_for_backward(q, k, v, out, stats)
        ctx.mask, ctx.heads, ctx.pitches = mask, heads, (qp, kp)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out, stats = ctx.saved_tensors
        mask, heads, (qp, kp) = ctx.mask, ctx.heads, ctx.pitches
        Fr, Tq, C = out.shape
        Tk = k.shape[1]
        grad_out = grad_out.float().contiguous()
        dq = torch.empty(Fr, Tq, C, device=q.device, dtype=torch.float32)
        dkv = torch.empty(2, Fr, Tk, C, device=q.device, dtype=torch.float32)
        nat.launch(q.device, nat.lib.sf_op_maskattn_backward, q.data_ptr(), qp, k.data_ptr(), v.data_ptr(), kp,
                   nat.ptr(mask.words if mask is not None else None), int(mask is not None and mask.per_head), out.data_ptr(), stats.data_ptr(),
                   grad_out.data_ptr(), dq.data_ptr(), C, dkv[0].data_ptr(), dkv[1].data_ptr(), C, Fr, Tq, Tk, heads, C // heads, 0)
        return dq, dkv[0], dkv[1], None, None


def masked_attention(q, k, v, mask: Optional[PackedAttentionMask] = None, heads: int = 8):
    """q ``[F, Tq, C]``, k and v ``[F, Tk, C]`` (fp32, head h in columns ``h * C / heads ...``) -> ``[F, Tq, C]``.  ``mask`` from
    ``pack_attention_mask``; ``None`` is unmasked attention (self-attention).  A query that sees no key gets zeros."""
    return MaskedAttentionFunction.apply(q, k, v, mask, heads)


class _OutProj(nn.Linear):
    """``out_proj`` under nn.MultiheadAttention's name and initialisation (its NonDynamicallyQuantizableLinear is a plain Linear)."""


class MaskedMultiheadAttention(nn.Module):
    """``nn.MultiheadAttention(embed_dim, num_heads, dropout, bias)`` on the HIP kernels: the same parameter names, shapes and
    initialisation (``in_proj_weight``, ``in_proj_bias``, ``out_proj.weight``, ``out_proj.bias``), so its state dict loads strictly both
    ways.  The projections are torch ``F.linear`` around ``MaskedAttentionFunction``.

    Refused by name: float masks, ``key_padding_mask``, ``need_weights=True``, ``dropout > 0`` in training mode, ``batch_first``,
    ``kdim`` / ``vdim``, ``add_bias_kv`` / ``add_zero_attn``, CPU tensors.  A fully hidden row gives zeros where torch gives NaN."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, bias: bool = True, add_bias_kv: bool = False,
                 add_zero_attn: bool = False, kdim=None, vdim=None, batch_first: bool = False):
        super().__init__()
        if batch_first:
            raise NotImplementedError("MaskedMultiheadAttention: batch_first is not supported (the reference's layers are sequence-first)")
        if (kdim is not None and kdim != embed_dim) or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError("MaskedMultiheadAttention: kdim / vdim other than embed_dim are not supported")
        if add_bias_kv or add_zero_attn:
            raise NotImplementedError("MaskedMultiheadAttention: add_bias_kv / add_zero_attn are not supported")
        if embed_dim <= 0 or num_heads <= 0 or embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        hd = embed_dim // num_heads
        if hd % 8 or not 8 <= hd <= 128:
            raise ValueError(f"the head width embed_dim / num_heads = {hd} must be a multiple of 8 in 8..128")
        self.embed_dim, self.num_heads, self.dropout, self.head_dim, self.batch_first = embed_dim, num_heads, float(dropout), hd, False
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = _OutProj(embed_dim, embed_dim, bias=bias)
        self._reset_parameters()

    def _reset_parameters(self) -> None:
        xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            constant_(self.in_proj_bias, 0.)
            constant_(self.out_proj.bias, 0.)

    @classmethod
    def from_torch(cls, mha: nn.MultiheadAttention) -> "MaskedMultiheadAttention":
        """A module that SHARES ``mha``'s parameters; raises for a configuration the kernels do not cover."""
        if not getattr(mha, "_qkv_same_embed_dim", True):
            raise NotImplementedError("MaskedMultiheadAttention: kdim / vdim other than embed_dim are not supported")
        new = cls(mha.embed_dim, mha.num_heads, dropout=mha.dropout, bias=mha.in_proj_bias is not None,
                  add_bias_kv=mha.bias_k is not None, add_zero_attn=mha.add_zero_attn, batch_first=mha.batch_first)
        new.in_proj_weight, new.in_proj_bias = mha.in_proj_weight, mha.in_proj_bias
        new.out_proj.weight, new.out_proj.bias = mha.out_proj.weight, mha.out_proj.bias
        new.train(mha.training)
        return new

    def _mask(self, attn_mask, Fr: int, Tq: int, Tk: int) -> Optional[PackedAttentionMask]:
        if attn_mask is None or isinstance(attn_mask, PackedAttentionMask):
            return attn_mask
        if attn_mask.dim() == 2 and tuple(attn_mask.shape) == (Tq, Tk):
            return pack_attention_mask(attn_mask[None].expand(Fr, Tq, Tk))
        if attn_mask.dim() == 3 and tuple(attn_mask.shape) == (Fr, Tq, Tk):
            return pack_attention_mask(attn_mask)
        if attn_mask.dim() == 3 and tuple(attn_mask.shape) == (Fr * self.num_heads, Tq, Tk):
            return pack_attention_mask(attn_mask, heads=self.num_heads)
        raise ValueError(f"attn_mask {tuple(attn_mask.shape)} is none of [Tq, Tk] = {(Tq, Tk)}, [F, Tq, Tk] = {(Fr, Tq, Tk)}, "
                         f"[F * heads, Tq, Tk] = {(Fr * self.num_heads, Tq, Tk)}")

    def forward(self, query, key, value, key_padding_mask=None, need_weights: bool = False, attn_mask=None):
        """query ``[Tq, F, C]``, key and value ``[Tk, F, C]`` -> ``(out [Tq, F, C], None)``."""
        if key_padding_mask is not None:
            raise NotImplementedError("MaskedMultiheadAttention: key_padding_mask is not supported (fold it into attn_mask)")
        if need_weights:
            raise NotImplementedError("MaskedMultiheadAttention: need_weights=True is not supported (the probabilities are never formed)")
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError("MaskedMultiheadAttention: dropout > 0 in training mode is not supported")
        if attn_mask is not None and not isinstance(attn_mask, PackedAttentionMask) and \
                not (isinstance(attn_mask, torch.Tensor) and attn_mask.dtype == torch.bool):
            raise TypeError("MaskedMultiheadAttention: float masks are not supported; attn_mask must be bool (True = hidden) or a "
                            "PackedAttentionMask")
        _need_gpu(query, "MaskedMultiheadAttention")
        if query.dim() != 3 or key.dim() != 3 or tuple(value.shape) != tuple(key.shape) or key.shape[1:] != query.shape[1:] or \
                query.shape[2] != self.embed_dim:
            raise ValueError(f"query [Tq, F, {self.embed_dim}], key and value [Tk, F, {self.embed_dim}]; got {tuple(query.shape)}, "
                             f"{tuple(key.shape)}, {tuple(value.shape)}")
        Tq, Fr, C = query.shape
        Tk = key.shape[0]
        mask = self._mask(attn_mask, Fr, Tq, Tk)
        w, b = self.in_proj_weight, self.in_proj_bias
        bias = (lambda i: None) if b is None else (lambda i: b[i * C:(i + 1) * C])
        if key is query and value is query:
            qkv = F.linear(query.transpose(0, 1), w, b)      # [F, T, 3 C]: the kernels read the three column ranges in place
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        else:
            q = F.linear(query.transpose(0, 1), w[:C], bias(0))
            if key is value:
                kv = F.linear(key.transpose(0, 1), w[C:], None if b is None else b[C:])
                k, v = kv[..., :C], kv[..., C:]
            else:
                k = F.linear(key.transpose(0, 1), w[C:2 * C], bias(1))
                v = F.linear(value.transpose(0, 1), w[2 * C:], bias(2))
        out = MaskedAttentionFunction.apply(q, k, v, mask, self.num_heads)
        return F.linear(out, self.out_proj.weight, self.out_proj.bias).transpose(0, 1), None


def use_native_attention(module: nn.Module) -> int:
    """Replace every compatible ``nn.MultiheadAttention`` below ``module`` (not ``module`` itself) by a ``MaskedMultiheadAttention``
    that shares its parameters; state-dict keys do not change.  An incompatible one (``batch_first``, ``kdim`` / ``vdim``, bias_kv,
    zero_attn, a head width the kernels do not take) stays as it is.  Returns the number replaced."""
    count = 0
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.MultiheadAttention:
                try:
                    new = MaskedMultiheadAttention.from_torch(child)
                except (NotImplementedError, ValueError):
                    continue
                setattr(parent, name, new)
                count += 1
    return count
