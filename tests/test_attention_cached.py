"""The temporal-attention kernels of a stream, alone (sf_op_attention_cached), against fp64 at their own precision floor.

Every kernel ``sf_launch_temporal_attention`` can choose is run on a caller-built KV-cache — spare capacity, a slot, a past, the position
in device memory, the table of a ragged call — and compared with tests/attention_oracle.py (written from the SfAttnArgs contract).  Every
cache row the contract does not name is NaN, so a kernel that reads one row too many, or the slab of another stream, shows as a NaN; the
context is written into a NaN-guarded buffer.  The bound is ``check_against_floor``: MARGIN times what the torch restatement of the same
sequence (fp32, on the operands the mode stores, output rounded as stored) loses against fp64.  Every case asserts the route the entry
reports, and ``ROUTES_REACHED`` below that the case lists reach every route.

Largest measured error / bound per route on an MI355X (0.25 = the restatement's own error: MARGIN is 4):

    single query, fp32 rows, 64 / 128 / 256 keys (routes 1, 2, 3)             0.260  0.250  0.259
    single query, bf16 whole lines, 64 / 128 keys (4, 5)                      0.250  0.250
    single query, bf16 lane = key, 64 / 128 / 256 keys (6, 7, 8)              0.250  0.250  0.250
    DMA-staged, bf16 rows (9)                                                 0.333
    MFMA, fp32 rows, 32 / 64 / 128 / 256 keys (11 .. 14), MFMA_ACC_MARGIN     0.252  0.189  0.252  0.437
    MFMA, bf16 rows, 32 / 64 / 128 / 256 keys (15 .. 18)                      0.250  0.267  0.324  0.257
    generic kernel, head_dim 32 / 72 / 128 (19)                               0.269

With MARGIN alone the MFMA kernel on fp32 rows reached 1.009 (Tq 3, Tk 8) and 1.007 (Tq 33, Tk 128) of the bound: the precision of
its bf16x3 products, see MFMA_ACC_MARGIN.  No case showed a wrong kernel.

Mutation check (not committed): with ``key < Tk - 1`` for ``key < Tk`` in sf_temporal_decode_lines_kernel 17 of the single-query and
probe tests fail; with the slab index ``bs`` replaced by ``b`` in the single-query kernels the six head_dim-64 table tests fail.
"""
import ctypes

import pytest
import torch

from tests import attention_oracle as AO
from tests.helpers import MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded

pytestmark = pytest.mark.gpu

N_TOK, HEADS = 3, 3            # 9 tasks per slab: with B = 2 or 3 the last workgroup of four waves is partial

# SfTemporalRoute (csrc/sf_common.h)
R_NONE, R_F32_1, R_F32_2, R_F32_4, R_LINES_1, R_LINES_2, R_BF16_1, R_BF16_2, R_BF16_4, R_DMA, R_DMA_PLANES = range(11)
R_MFMA_ACC, R_MFMA_BF16, R_GENERIC = 11, 15, 19          # + 0 .. 3: 32 / 64 / 128 / 256 keys
ALL_ROUTES = set(range(1, 20)) - {R_DMA_PLANES}           # hi + lo planes are whole-clip only: reached through sf_op_attention


def expected_route(mode, hd, Tq, Tk, lane_key=False, decode_off=False):
    """The dispatch as the header documents it, restated: what each case must report."""
    if hd != 64:
        return R_GENERIC
    if Tq == 1 and Tk <= 256 and not decode_off:
        kp = (Tk + 63) // 64
        if mode == 1:
            return {1: R_F32_1, 2: R_F32_2}.get(kp, R_F32_4)
        if kp <= 2 and not lane_key:
            return {1: R_LINES_1, 2: R_LINES_2}[kp]
        return {1: R_BF16_1, 2: R_BF16_2}.get(kp, R_BF16_4)
    if mode == 0 and Tq <= 16 and Tk <= 32:
        return R_DMA
    nt2 = (Tk + 31) // 32
    return (R_MFMA_ACC if mode == 1 else R_MFMA_BF16) + (0 if nt2 <= 1 else 1 if nt2 <= 2 else 2 if nt2 <= 4 else 3)


# ---- the case lists -----------------------------------------------------------------------------------------------------------------
SINGLE_TK = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256]
DEVICE_TK = [64, 65, 128, 129, 192, 193]                     # one on each side of 64, 128 and 192
TAB_SLABS, TAB_STREAMS = 5, (4, 0, 2)
TAB_TK = [(1, 63, 64), (65, 127, 128), (129, 200, 256)]
DEVICE_HD = [64, 72, 32]
PROBE_KEYS = [0, 7, 8, 63, 64, 127, 128, 255]
PROBE_TK = [64, 128, 200, 256]
CHUNK_DMA = [(2, 17), (3, 8), (5, 32), (16, 32)]              # bf16: the DMA-staged kernel; accurate: the 32-key MFMA instance
# one value on each side of each MAXNT2 step; (17, 32): more than one query tile on 32 keys, the bf16 32-key MFMA instance
CHUNK_MFMA = [(2, 33), (16, 64), (17, 65), (33, 128), (16, 129), (8, 200), (16, 256), (17, 32)]
CHUNK_GENERIC = [(3, 8), (16, 48), (17, 33), (33, 100)]
CHUNK_GENERIC_HD = [72, 128]


def host_tk(tk):
    """The largest host Tk that selects the instance of ``tk`` keys."""
    return 64 * {1: 1, 2: 2, 3: 4, 4: 4}[(tk + 63) // 64]


def _routes_of_the_lists():
    r = set()
    for tk in SINGLE_TK:
        r |= {expected_route(1, 64, 1, tk), expected_route(0, 64, 1, tk), expected_route(0, 64, 1, tk, lane_key=True),
              expected_route(0, 64, 1, tk, decode_off=True)}
    for tk in DEVICE_TK + [max(t) for t in TAB_TK]:
        r |= {expected_route(m, hd, 1, host_tk(tk)) for m in (0, 1) for hd in DEVICE_HD}
    for tq, tk in CHUNK_DMA + CHUNK_MFMA:
        r |= {expected_route(m, 64, tq, tk) for m in (0, 1)}
    return r


ROUTES_REACHED = _routes_of_the_lists()
assert ROUTES_REACHED >= ALL_ROUTES, sorted(ALL_ROUTES - ROUTES_REACHED)      # a dispatch change cannot leave an instance without a case


# ---- inputs, the call, the check ----------------------------------------------------------------------------------------------------
def make_cache(seed, slabs, cap, hd, live):
    """Seeded randn * 1.5 plus one spiky column; ``live[s]`` rows of slab s are named by the call, every other row is NaN."""
    D = HEADS * hd
    c = torch.randn(slabs, cap, N_TOK, 3 * D, generator=torch.Generator().manual_seed(seed)) * 1.5
    c[..., 5] += 6.0
    for s in range(slabs):
        c[s, live.get(s, 0):] = float("nan")
    return c


def run(cache, hd, mode, B, Tq, Tk, q_t0, t_past, causal, pos=None, tab=None):
    """One call of the entry: (return code, route, waves per workgroup, guard buffer, its view)."""
    import streamformer_amd._native as nat
    dev = gpu_device()
    slabs, cap, N, D3 = cache.shape
    c = cache.to(dev).contiguous()
    buf, view = guarded(dev, B * Tq * N, D3 // 3)
    nb = nat.lib.sf_op_attention_cached_workspace_bytes(slabs, cap, N, HEADS, hd, B, Tq)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    pos_t = None if pos is None else torch.tensor(list(pos), dtype=torch.int32, device=dev)
    tab_t = None if tab is None else torch.tensor([[s, 12345, slot, tk] for s, slot, tk in tab], dtype=torch.int32, device=dev)      # t_row: unused
    route, waves = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = nat.lib.sf_op_attention_cached(c.data_ptr(), view.data_ptr(), slabs, cap, N, HEADS, hd, mode, B, Tq, Tk, q_t0, t_past, int(causal),
                                        nat.ptr(pos_t), nat.ptr(tab_t), ctypes.byref(route), ctypes.byref(waves), ws.data_ptr(), nb,
                                        nat.current_stream_handle(dev))
    torch.cuda.synchronize()
    return rc, route.value, waves.value, buf, view


def run_ok(cache, hd, mode, route, *args, **kw):
    import streamformer_amd._native as nat
    rc, got_route, waves, buf, view = run(cache, hd, mode, *args, **kw)
    nat.check(rc)
    assert got_route == route, (got_route, route)
    return read_guarded(buf, view), waves


# The MFMA kernel on fp32 rows (routes 11 .. 14) computes both products as bf16x3: q, k, the probabilities and v each enter as a hi + lo
# bf16 pair, a 16-bit significand, where the restatement keeps fp32 operands and rounds to 16 bits once, at the output.  Four more
# roundings of the output's own size, so four times the margin.  Measured on the MI355X with MARGIN: 1.009 of the bound at (Tq 3, Tk 8)
# and 1.007 at (33, 128), 0.50 .. 0.76 on the other cases up to there.  A CPU emulation of the three-product arithmetic (fp32
# accumulation, exp2, the same inputs) loses exactly as much, 4.04 and 4.03 floors, and 6.2 floors at (16, 256); the split of q and k
# alone gives 2.3, 4.0 and 6.7 floors: it is the scores' precision.  The single-query kernel on fp32 rows multiplies in fp32: 0.26.
MFMA_ACC_MARGIN = 4 * MARGIN


def margin_of(route):
    return MFMA_ACC_MARGIN if R_MFMA_ACC <= route < R_MFMA_ACC + 4 else MARGIN


class Ref:
    """fp64 reference and fp32 floor of one case, computed once and shared by every route that runs the case."""

    def __init__(self, cache, mode, *args, **kw):
        self.want = AO.cached_attention_want(cache, mode, HEADS, *args, **kw)
        self.floor = AO.cached_attention_floor(cache, mode, HEADS, *args, **kw)
        self.bound = MARGIN * fp32_floor(self.floor, self.want)         # of every route but the MFMA kernel on fp32 rows

    def check(self, what, route, got):
        print(f"ROUTE {route} {maxabs(got, self.want) / (self.bound * margin_of(route) / MARGIN):.3f}")
        check_against_floor(f"{what} route {route}", got, self.floor, self.want, margin=margin_of(route))


# ---- 1. single query, position by value -----------------------------------------------------------------------------------------------
def _single_cases(Tk):
    """(cap, q_t0, causal): plain streaming in a full and in a spare cache, and a wrapped window (the query mid-ring)."""
    return [(cap, q_t0, causal) for cap, q_t0 in ((Tk, Tk - 1), (Tk + 3, Tk - 1), (Tk, Tk // 2)) for causal in (1, 0)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Tk", SINGLE_TK)
def test_single_query_by_value(Tk, mode, switches):
    B = 3
    cases = []
    for cap, q_t0, causal in _single_cases(Tk):
        cache = make_cache(Tk * 7 + cap, B, cap, 64, {b: Tk for b in range(B)})
        args = (B, 1, Tk, q_t0, Tk - 1, causal)
        cases.append((cache, args, Ref(cache, mode, *args)))
    results = []
    # bf16 mode: the whole-line kernel, then the lane = key kernel, then the multi-query kernels on the same inputs
    for sw, kw in ((None, {}), ("SF_TEMPORAL_DECODE_LANE_KEY", dict(lane_key=True)), ("SF_DISABLE_TEMPORAL_DECODE", dict(decode_off=True))):
        if sw:
            if mode == 1:
                break
            switches(sw)
        route = expected_route(mode, 64, 1, Tk, **kw)
        outs = []
        for cache, args, ref in cases:
            got, _ = run_ok(cache, 64, mode, route, *args)
            ref.check(f"single Tk={Tk} cap={cache.shape[1]} q_t0={args[3]} causal={args[5]}", route, got)
            outs.append(got)
        results.append(outs)
    for other in results[1:]:                       # the routes agree with each other to the bound each of them meets
        for a, b, (_, _, ref) in zip(results[0], other, cases):
            assert maxabs(a, b) <= ref.bound, (Tk, maxabs(a, b), ref.bound)


# ---- 2. single query, position from device memory -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hd", DEVICE_HD)
@pytest.mark.parametrize("tk", DEVICE_TK)
def test_single_query_pos_dev(tk, hd, mode):
    """{slot, tk} in device memory; the by-value arguments name another legal position (row 0, one visible key, the instance's largest Tk)."""
    B, Tk = 2, host_tk(tk)
    cap = Tk + 3
    route = expected_route(mode, hd, 1, Tk)
    for slot in (tk - 1, tk // 2):
        cache = make_cache(tk * 11 + slot + hd, B, cap, hd, {b: tk for b in range(B)})
        for causal in (1, 0):
            args = (B, 1, Tk, 0, 0, causal)
            ref = Ref(cache, mode, *args, pos=(slot, tk))
            got, _ = run_ok(cache, hd, mode, route, *args, pos=(slot, tk))
            ref.check(f"pos_dev tk={tk} slot={slot} hd={hd} causal={causal}", route, got)
            if causal:                              # the by-value position gives something else: the device values were followed
                assert maxabs(AO.cached_attention_want(cache, mode, HEADS, B, 1, tk, 0, 0, 1), ref.want) > 0.1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hd", DEVICE_HD)
@pytest.mark.parametrize("tks", TAB_TK, ids=lambda t: "-".join(map(str, t)))
def test_single_query_table(tks, hd, mode):
    """A ragged call: row b of the call reads slab tab[b].stream at its own slot and key count; the other slabs are NaN."""
    B, Tk = 3, max(tks)
    cap = Tk + 3
    route = expected_route(mode, hd, 1, Tk)
    tab = [(s, (tk - 1 if i % 2 == 0 else tk // 2), tk) for i, (s, tk) in enumerate(zip(TAB_STREAMS, tks))]
    cache = make_cache(sum(tks) + hd, TAB_SLABS, cap, hd, {s: tk for s, _, tk in tab})
    for causal in (1, 0):
        args = (B, 1, Tk, 0, 0, causal)
        ref = Ref(cache, mode, *args, tab=tab)
        got, _ = run_ok(cache, hd, mode, route, *args, tab=tab)
        ref.check(f"tab tk={tks} hd={hd} causal={causal}", route, got)
    # context row b is the result of slab tab[b].stream alone
    for b, (s, slot, tk) in enumerate(tab):
        one = make_cache(0, 1, cap, hd, {0: tk})
        one[0] = cache[s]
        alone = AO.cached_attention_want(one, mode, HEADS, 1, 1, tk, slot, tk - 1, False)
        assert maxabs(ref.want[b * N_TOK:(b + 1) * N_TOK], alone) < 1e-12


# ---- 3. every key counts ----------------------------------------------------------------------------------------------------------------
def _probe_cache(Tk, cap, hd, j, B=2):
    """Key j dominates every (sequence, head): k_j = 3 q.  V_j is a constant row that no other row resembles."""
    D = HEADS * hd
    cache = make_cache(Tk + j, B, cap, hd, {b: Tk for b in range(B)})
    cache[:, j, :, D:2 * D] = 3.0 * cache[:, Tk - 1, :, :D]
    d = torch.arange(D)
    cache[:, j, :, 2 * D:] = 0.5 + 0.125 * ((d[None, None, :] + torch.arange(N_TOK)[None, :, None] * 5 + torch.arange(B)[:, None, None] * 3) % 16)
    return cache


PROBE_ROUTES = [(1, 64, {}), (0, 64, {}), (0, 64, dict(lane_key=True)), (0, 72, {}), (1, 72, {})]


@pytest.mark.parametrize("mode,hd,kw", PROBE_ROUTES, ids=["f32", "bf16", "bf16-lane-key", "generic-bf16", "generic-f32"])
@pytest.mark.parametrize("Tk", PROBE_TK)
def test_every_key_counts(Tk, mode, hd, kw, switches):
    """One dominant key per probe, at the edges of the kernels' key layouts: a dropped, duplicated or mislocated key is an O(1) error."""
    if kw:
        switches("SF_TEMPORAL_DECODE_LANE_KEY")
    B, cap, D = 2, Tk + 3, HEADS * hd
    route = expected_route(mode, hd, 1, Tk, **kw)
    for j in sorted({k for k in PROBE_KEYS if k < Tk} | {Tk - 1}):
        cache = _probe_cache(Tk, cap, hd, j)
        args = (B, 1, Tk, Tk - 1, Tk - 1, 1)
        ref = Ref(cache, mode, *args)
        _, probs = AO.cached_attention_want(cache, mode, HEADS, *args, return_probs=True)
        assert min(float(p[..., j].min()) for p in probs) >= 1 - 1e-6, (Tk, j)      # from the reference alone
        v_j = AO.stored_operands(cache, mode)[:, j, :, 2 * D:].reshape(B * N_TOK, D)
        assert maxabs(ref.want, v_j) <= 1e-4
        got, _ = run_ok(cache, hd, mode, route, *args)
        ref.check(f"probe Tk={Tk} key={j} hd={hd}", route, got)
        assert maxabs(got, v_j) <= ref.bound + 1e-4, (Tk, j, maxabs(got, v_j))


# ---- 4. chunked prefill with a past -----------------------------------------------------------------------------------------------------
def _chunk(Tq, Tk, hd, mode, route):
    B, cap = 2, Tk + 2
    cache = make_cache(Tq * 31 + Tk + hd, B, cap, hd, {b: Tk for b in range(B)})
    waves = []
    for causal in (1, 0):
        args = (B, Tq, Tk, Tk - Tq, Tk - Tq, causal)
        ref = Ref(cache, mode, *args)
        got, w = run_ok(cache, hd, mode, route, *args)
        ref.check(f"chunk Tq={Tq} Tk={Tk} hd={hd} causal={causal}", route, got)
        waves.append(w)
    return waves[0]


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_prefill_short(mode):
    for Tq, Tk in CHUNK_DMA:
        assert _chunk(Tq, Tk, 64, mode, expected_route(mode, 64, Tq, Tk)) == 4


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_prefill_mfma(mode):
    waves = {(Tq, Tk): _chunk(Tq, Tk, 64, mode, expected_route(mode, 64, Tq, Tk)) for Tq, Tk in CHUNK_MFMA}
    print("waves per workgroup:", waves)
    assert waves[(2, 33)] == 4 and waves[(17, 32)] == 4
    if mode == 1:       # fp32 rows keep V^T as hi + lo patches: from 129 keys on four of them no longer fit, the launcher halves the waves
        assert all(waves[c] < 4 for c in CHUNK_MFMA if c[1] >= 129), waves
    else:
        assert all(w >= 2 for w in waves.values())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hd", CHUNK_GENERIC_HD)
def test_chunked_prefill_generic(hd, mode):
    for Tq, Tk in CHUNK_GENERIC:
        _chunk(Tq, Tk, hd, mode, R_GENERIC)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
#            B  Tq Tk  q_t0 t_past  cap  hd  pos       tab                      message
REFUSALS = [(2, 2, 8, 7, 6, 8, 64, None, None, b"leave the cache"),
            (2, 1, 9, 7, 7, 8, 64, None, None, b"Tk 9 > cap 8"),
            (2, 2, 8, 0, 6, 8, 64, None, [(0, 0, 4), (1, 0, 4)], b"Tq 2 != 1"),
            (2, 2, 8, 0, 6, 8, 64, (3, 4), None, b"Tq 2 != 1"),
            (3, 1, 8, 7, 7, 8, 64, None, None, b"B 3 > 2"),
            (2, 1, 8, 7, 7, 8, 12, None, None, b"head_dim"),
            (2, 1, 8, 0, 0, 8, 64, (3, 9), None, b"device position"),
            (2, 1, 8, 0, 0, 8, 64, (8, 4), None, b"device position"),
            (2, 1, 8, 0, 0, 8, 64, None, [(0, 3, 4), (2, 3, 4)], b"device position"),
            (2, 2, 300, 298, 298, 300, 64, None, None, b"no temporal attention kernel")]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[-1].decode().replace(" ", "-"))
def test_refusals(case):
    import streamformer_amd._native as nat
    B, Tq, Tk, q_t0, t_past, cap, hd, pos, tab, msg = case
    cache = make_cache(1, 2, cap, hd if hd % 8 == 0 else 16, {0: cap, 1: cap})
    rc, route, waves, buf, view = run(cache, hd, 1, B, Tq, Tk, q_t0, t_past, 1, pos=pos, tab=tab)
    assert rc == nat.SF_ERR_INVALID and msg in nat.lib.sf_last_error(), (rc, nat.lib.sf_last_error())
    assert route == R_NONE and waves == 0
    assert torch.isnan(buf.cpu()).all(), "a refused call wrote its output"


def test_refuses_device_position_on_a_route_that_ignores_it(switches):
    import streamformer_amd._native as nat
    switches("SF_DISABLE_TEMPORAL_DECODE")
    cache = make_cache(2, 2, 8, 64, {0: 8, 1: 8})
    rc, route, _, buf, _ = run(cache, 64, 0, 2, 1, 8, 0, 0, 1, pos=(3, 4))
    assert rc == nat.SF_ERR_INVALID and b"does not read tab / pos_dev" in nat.lib.sf_last_error()
    assert route == R_NONE and torch.isnan(buf.cpu()).all()
