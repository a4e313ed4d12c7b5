"""Oracles of the masked-attention training path (streamformer_amd/masked_attention.py), on the CPU in any dtype.

  attention            the plain torch sequence (scores, -inf fill, softmax, P V) with torch autograd behind it: in fp64 it is the oracle,
                       in fp32 the precision floor of the kernels.  A query without a visible key gets zeros and passes no gradient
                       (torch's own softmax gives NaN there; the kernels define zeros).
  recompute_backward   the backward as the kernels do it: P recomputed from the row statistics, delta = rowsum(dO o ctx).
Masks are bool, True = hidden: [F, Q, HW] (shared by the heads) or [F, heads, Q, HW]; None hides nothing.
"""
import torch


MASKS = ("none", "clear", "random", "query", "tile", "key", "last", "runs", "heads")


def make_mask(kind, rs, Fr, heads, Q, HW):
    """The mask cases of the tests as numpy bool ([F, Q, HW]; "heads": [F, heads, Q, HW]), None for "none".
      clear   nothing hidden                       random  about half hidden
      query   one query sees no key                key     one key is seen by no query
      tile    the second 16-key tile (the first, below 32 keys) hidden from the first 16 queries and from nobody else
      last    only the last key visible            runs    hidden runs of 3..11 keys across every word boundary
      heads   random, drawn separately per head (one query of head 0 and one key of head 1 hidden altogether)"""
    import numpy as np
    if kind == "none":
        return None
    m = np.zeros((Fr, Q, HW), bool)
    if kind == "random":
        m = rs.random_sample((Fr, Q, HW)) < 0.5
    elif kind == "query":
        m = rs.random_sample((Fr, Q, HW)) < 0.3
        m[:, Q // 2] = True
    elif kind == "key":
        m = rs.random_sample((Fr, Q, HW)) < 0.3
        m[:, :, HW // 2] = True
    elif kind == "tile":
        k0 = 16 if HW >= 32 else 0
        m[:, :16, k0:k0 + 16] = True
    elif kind == "last":
        m[:] = True
        m[:, :, HW - 1] = False
    elif kind == "runs":
        for b in range(0, HW + 32, 32):
            for qq in range(Q):
                lo, n = b - 1 - (qq % 5), 3 + (qq % 9)
                m[:, qq, max(lo, 0):max(min(lo + n, HW), 0)] = True
        m[1:] = np.roll(m[1:], 1, axis=1)
    elif kind == "heads":
        m = rs.random_sample((Fr, heads, Q, HW)) < 0.5
        m[:, 0, Q // 2] = True
        m[:, heads - 1, :, HW // 2] = True
    return m


def split(t, heads):
    """[F, T, C] -> [F, heads, T, C / heads]"""
    Fr, T, C = t.shape
    return t.reshape(Fr, T, heads, C // heads).transpose(1, 2)


def merge(t):
    """[F, heads, T, hd] -> [F, T, C]"""
    Fr, H, T, hd = t.shape
    return t.transpose(1, 2).reshape(Fr, T, H * hd)


def head_mask(mask, Fr, heads, Q, HW):
    """-> bool [F, heads, Q, HW]"""
    if mask is None:
        return torch.zeros(Fr, heads, Q, HW, dtype=torch.bool)
    m = torch.as_tensor(mask)
    return (m[:, None] if m.dim() == 3 else m).expand(Fr, heads, Q, HW)


def attention(q, k, v, mask, heads):
    """-> (ctx [F, Q, C], stats [F, heads, Q]: log-sum-exp of the scaled scores over the visible keys, +inf without one)"""
    Fr, Q, C = q.shape
    HW = k.shape[1]
    m = head_mask(mask, Fr, heads, Q, HW)
    dead = m.all(-1, keepdim=True)
    s = (split(q, heads) @ split(k, heads).transpose(-1, -2)) / ((C // heads) ** 0.5)
    s = s.masked_fill(m, float("-inf")).masked_fill(dead, 0.0)
    p = torch.softmax(s, -1).masked_fill(m | dead, 0.0)
    stats = torch.logsumexp(s, -1).masked_fill(dead[..., 0], float("inf"))
    return merge(p @ split(v, heads)), stats


def autograd_backward(q, k, v, mask, heads, d_ctx):
    """-> (ctx, stats, dq, dk, dv) by torch autograd through `attention`, in the dtype of the inputs"""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ctx, stats = attention(q, k, v, mask, heads)
    dq, dk, dv = torch.autograd.grad(ctx, (q, k, v), d_ctx)
    return ctx.detach(), stats.detach(), dq, dk, dv


def recompute_backward(q, k, v, mask, heads, ctx, stats, d_ctx):
    """-> (dq, dk, dv) from the saved ctx and stats alone, the kernels' formulas"""
    Fr, Q, C = q.shape
    HW = k.shape[1]
    scale = 1.0 / ((C // heads) ** 0.5)
    m = head_mask(mask, Fr, heads, Q, HW)
    qh, kh, vh, do = split(q, heads), split(k, heads), split(v, heads), split(d_ctx, heads)
    delta = (do * split(ctx, heads)).sum(-1, keepdim=True)
    p = torch.exp(qh @ kh.transpose(-1, -2) * scale - stats[..., None]).masked_fill(m, 0.0)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ vh.transpose(-1, -2) - delta)
    return merge(ds @ kh) * scale, merge(ds.transpose(-1, -2) @ qh) * scale, merge(dv)
