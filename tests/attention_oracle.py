"""Reference of the temporal attention over a KV-cache (not a test file), written from the SfAttnArgs contract (csrc/sf_common.h), not
from the kernels.

The cache is ``[slabs, cap, N, 3 D]`` with q | k | v per row.  For sequence (b, n):

  * query t < Tq is row ``q_t0 + t`` of slab s(b); keys and values are rows ``0 .. Tk_b - 1`` of that slab;
  * causal: key j is visible to query t iff ``j <= t_past + t``;
  * by value: s(b) = b, Tk_b = Tk;
  * ``pos = (slot, tk)`` (the position in device memory): the query row is ``slot``, tk keys, all of them visible;
  * ``tab = [(stream, slot, tk), ...]`` (a ragged call): s(b) = stream, and the same per row; the context row stays row b;
  * the scale is ``head_dim ** -0.5``.

Only the rows the contract names are indexed, so the rest of the cache may hold anything (NaN included).  Everything runs in the dtype of
``cache``: fp64 gives the reference, fp32 the precision floor (``cached_attention_floor``).
"""
import torch

from tests.oracle_ops import bf16_round


def positions(B, Tq, Tk, q_t0, t_past, causal, pos=None, tab=None):
    """Per sequence b: (slab, first query row, keys, t_past, causal) as the contract resolves them."""
    if tab is not None:
        assert Tq == 1 and len(tab) == B
        return [(int(s), int(slot), int(tk), int(tk) - 1, False) for s, slot, tk in tab]
    if pos is not None:
        assert Tq == 1
        slot, tk = pos
        return [(b, int(slot), int(tk), int(tk) - 1, False) for b in range(B)]
    return [(b, q_t0, Tk, t_past, bool(causal)) for b in range(B)]


def cached_attention(cache, heads, B, Tq, Tk, q_t0, t_past, causal, pos=None, tab=None, return_probs=False):
    """Context rows [B * Tq * N, D] (rows (b, t, n)); with ``return_probs`` also the probabilities, one [N, heads, Tq, Tk_b] per b."""
    slabs, cap, N, D3 = cache.shape
    D = D3 // 3
    hd = D // heads
    out = cache.new_zeros(B, Tq, N, D)
    probs = []
    for b, (s, q0, tk, past, caus) in enumerate(positions(B, Tq, Tk, q_t0, t_past, causal, pos, tab)):
        assert 0 <= s < slabs and 0 <= q0 and q0 + Tq <= cap and 1 <= tk <= cap
        q = cache[s, q0:q0 + Tq, :, :D].reshape(Tq, N, heads, hd)
        k = cache[s, :tk, :, D:2 * D].reshape(tk, N, heads, hd)
        v = cache[s, :tk, :, 2 * D:].reshape(tk, N, heads, hd)
        sc = torch.einsum("tnhd,jnhd->nhtj", q, k) * hd ** -0.5
        if caus:
            j = torch.arange(tk)
            t = torch.arange(Tq)
            sc = sc.masked_fill(~(j[None, :] <= past + t[:, None]), float("-inf"))
        p = sc.softmax(dim=-1)
        probs.append(p)
        out[b] = torch.einsum("nhtj,jnhd->tnhd", p, v).reshape(Tq, N, D)
    out = out.reshape(B * Tq * N, D)
    return (out, probs) if return_probs else out


def stored_operands(cache, mode):
    """The cache as the compute mode keeps it in a stream, in fp32: bf16-rounded rows in bf16 mode (0), the fp32 rows in the accurate mode (1)."""
    c = cache.float()
    return bf16_round(c) if mode == 0 else c


def round_output(o, mode):
    """The context as the kernels store it: one bf16 rounding in bf16 mode, a hi + lo bf16 pair in the accurate mode."""
    hi = bf16_round(o)
    return hi if mode == 0 else hi + bf16_round(o - hi)


def cached_attention_floor(cache, mode, heads, B, Tq, Tk, q_t0, t_past, causal, pos=None, tab=None):
    """The torch restatement for the precision floor: the same sequence in fp32 on the operands the mode stores, output rounded as stored."""
    o = cached_attention(stored_operands(cache, mode), heads, B, Tq, Tk, q_t0, t_past, causal, pos, tab)
    return round_output(o, mode)


def cached_attention_want(cache, mode, heads, B, Tq, Tk, q_t0, t_past, causal, pos=None, tab=None, return_probs=False):
    """The fp64 reference on the operands the mode stores."""
    return cached_attention(stored_operands(cache, mode).double(), heads, B, Tq, Tk, q_t0, t_past, causal, pos, tab, return_probs)
