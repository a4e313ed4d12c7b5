"""CPU: the cached-attention reference (tests/attention_oracle.py) against ``O._mha`` with an independently built mask."""
import torch

from oracle import streamformer_oracle as O
from tests import attention_oracle as AO
from tests.helpers import maxabs, randn

HEADS, HD, N = 3, 8, 3
D = HEADS * HD


def _mha_rows(q, k, v, mask):
    """q [Tq, N, D], k / v [Tk, N, D] -> [Tq * N, D] through O._mha (sequences = tokens)."""
    out = O._mha(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), HEADS, mask)[0]      # [N, Tq, D]
    return out.transpose(0, 1).reshape(-1, D)


def test_whole_clip_is_plain_causal_attention():
    B, L = 2, 5
    cache = randn(1, B, L, N, 3 * D).double()
    got = AO.cached_attention(cache, HEADS, B, L, L, 0, 0, True)
    mask = torch.tril(torch.ones(L, L, dtype=torch.bool))
    for b in range(B):
        q, k, v = cache[b].split(D, dim=-1)
        assert maxabs(got.reshape(B, L * N, D)[b], _mha_rows(q, k, v, mask)) < 1e-13
    full = AO.cached_attention(cache, HEADS, B, L, L, 0, 0, False)
    q, k, v = cache[1].split(D, dim=-1)
    assert maxabs(full.reshape(B, L * N, D)[1], _mha_rows(q, k, v, None)) < 1e-13
    assert maxabs(full, got) > 1e-3


def test_chunked_prefill_with_a_past():
    B, Tq, Tk, cap = 2, 3, 8, 10
    cache = randn(2, B, cap, N, 3 * D).double()
    cache[:, Tk:] = float("nan")                       # rows the contract does not name
    got = AO.cached_attention(cache, HEADS, B, Tq, Tk, Tk - Tq, Tk - Tq, True)
    assert not torch.isnan(got).any()
    mask = torch.tril(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=Tk - Tq)      # query t sees keys 0 .. (Tk - Tq) + t
    assert mask[0].sum() == Tk - Tq + 1 and mask[-1].all()
    for b in range(B):
        q, k, v = cache[b, :Tk].split(D, dim=-1)
        assert maxabs(got.reshape(B, Tq * N, D)[b], _mha_rows(q[Tk - Tq:], k, v, mask)) < 1e-13


def test_wrapped_window_ring_order_equals_time_order():
    cap, seen = 6, 9                                   # frames 3 .. 8 are held; frame f sits in slot f % cap
    frames = randn(3, seen, N, 3 * D).double()
    ring = torch.empty(1, cap, N, 3 * D, dtype=torch.float64)
    for f in range(seen - cap, seen):
        ring[0, f % cap] = frames[f]
    slot = (seen - 1) % cap
    got = AO.cached_attention(ring, HEADS, 1, 1, cap, slot, cap - 1, True)
    q, k, v = frames[seen - cap:].split(D, dim=-1)      # time order: the query is the last frame and sees every key
    want = _mha_rows(q[-1:], k, v, None)
    assert maxabs(got, want) < 1e-13
    # the device-side forms of the same position
    assert torch.equal(AO.cached_attention(ring, HEADS, 1, 1, cap, 0, 0, True, pos=(slot, cap)), got)
    five = torch.full((5, cap, N, 3 * D), float("nan"), dtype=torch.float64)
    five[3] = ring[0]
    five[1, :2] = frames[:2]
    tab = AO.cached_attention(five, HEADS, 2, 1, cap, 0, 0, True, tab=[(3, slot, cap), (1, 1, 2)])
    assert torch.equal(tab[:N], got) and not torch.isnan(tab).any()
    q, k, v = frames[:2].split(D, dim=-1)
    assert maxabs(tab[N:], _mha_rows(q[1:2], k, v, None)) < 1e-13


def test_floor_restatement_rounds_operands_and_output_as_stored():
    cache = randn(4, 1, 7, N, 3 * D) * 1.5
    args = (HEADS, 1, 1, 7, 6, 6, True)
    for mode, rel in ((0, 2.0 ** -8), (1, 2.0 ** -16)):
        want = AO.cached_attention_want(cache, mode, *args)
        floor = AO.cached_attention_floor(cache, mode, *args)
        assert want.dtype == torch.float64 and floor.dtype == torch.float32
        assert 0 < maxabs(floor, want) <= rel * float(want.abs().max())
    assert torch.equal(AO.cached_attention_floor(cache, 0, *args), AO.cached_attention_floor(cache, 0, *args).bfloat16().float())
    assert maxabs(AO.cached_attention_want(cache, 0, *args), AO.cached_attention_want(cache, 1, *args)) > 1e-4      # operand rounding is in `want`
