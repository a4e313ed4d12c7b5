"""The native online-action detector on the MI355X: its attention kernel against fp64, the whole detector against the fp64 restatement
of the stream path (tests/oad_oracle.py) and the reference's stored scores (tests/golden/f20_oad.npz), the ring wrap, stream
independence, one full-width case and the streaming wrapper.

Tolerances follow tests/test_connector.py / test_text_tower.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds —
the error, against fp64, of the same operator sequence in torch at the operand precision of the mode (bf16_operands="x3" for the accurate
mode, True for the bf16 mode; plain fp32 for the kernel alone) — and never less than one fp32 rounding of the result.  The floor is
computed here, on the CPU, from the inputs; never from the code under test.
"""
import ctypes as C
import functools
import itertools

import pytest
import torch

from tests import oad_oracle as OO
from tests.helpers import MARGIN, fp32_floor, frames, gpu_device, maxabs, randn, small_cfg

pytestmark = pytest.mark.gpu

MODES = {"fp32": "x3", "bf16": True}
NINF = float("-inf")


# ------------------------------------------------------------------------------------------------
# 1. sf_op_oad_attention
# ------------------------------------------------------------------------------------------------
def _attention_ref(q, k, v, starts, kpos, vpos, mask, heads, causal):
    """q [Sq, Tq, D] (Sq = 1: shared), k / v [S, Tk, D] by SLOT, starts [S], kpos / vpos [Tk, D] or None, mask [S, Tk] or None -> [S, Tq, D] in
    q's dtype; a query without a visible key gets zeros."""
    S, Tk, _ = k.shape
    out = []
    for s in range(S):
        order = [(starts[s] + j) % Tk for j in range(Tk)]
        ks, vs = k[s][order], v[s][order]
        if kpos is not None:
            ks, vs = ks + kpos, vs + vpos
        if mask is not None:      # a masked key contributes exactly zero whatever it holds
            dead = mask[s] == NINF
            ks, vs = ks.masked_fill(dead[:, None], 0.0), vs.masked_fill(dead[:, None], 0.0)
        o = OO.attention(q[s if q.shape[0] > 1 else 0], ks, vs, heads, mask=None if mask is None else mask[s], causal=causal)
        out.append(torch.nan_to_num(o, nan=0.0))
    return torch.stack(out)


def _attention_call(nat, dev, q, k, v, starts, kpos, vpos, mask, heads, hd, causal):
    S, Tk, D = k.shape
    Tq = q.shape[1]
    ctx = torch.full((S * Tq + 1, D), float("nan"), device=dev)
    t = [None if x is None else x.to(dev).contiguous() for x in (q, k, v, kpos, vpos, mask)]
    st = None if starts is None else (C.c_int32 * S)(*starts)
    nat.check(nat.lib.sf_op_oad_attention(t[0].data_ptr(), q.shape[0], t[1].data_ptr(), t[2].data_ptr(), st, nat.ptr(t[3]), nat.ptr(t[4]), nat.ptr(t[5]),
                                          ctx.data_ptr(), S, Tq, Tk, heads, hd, int(causal), nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    out = ctx.cpu()
    assert torch.isnan(out[S * Tq:]).all(), "the guard row was written"
    assert not torch.isnan(out[:S * Tq]).any(), "output elements left unwritten"
    return out[:S * Tq].reshape(S, Tq, D)


@pytest.mark.parametrize("Tq,Tk,causal", [(1, 1, False), (5, 7, False), (16, 64, False), (33, 130, False), (6, 6, True), (32, 32, True)])
@pytest.mark.parametrize("hd", [8, 32, 72, 256])
def test_attention_kernel_vs_fp64(hd, Tq, Tk, causal):
    import streamformer_amd._native as nat
    dev = gpu_device()
    heads = 2
    D = heads * hd
    leads = sorted({0, min(3, Tk - 1), Tk - 1})
    rings = [None] + sorted({0, min(1, Tk - 1), Tk - 1})
    worst = 0.0
    for S, shared in itertools.product((1, 3), (True, False)):
        seed = 2100 + hd + 7 * Tq + 3 * S + int(shared)
        q = randn(seed, 1 if shared else S, Tq, D)
        k, v = randn(seed + 1, S, Tk, D), randn(seed + 2, S, Tk, D)
        kpos, vpos = 0.5 * randn(seed + 3, Tk, D), 0.5 * randn(seed + 4, Tk, D)
        for lead, ring in itertools.product(leads, rings):
            mask = None
            if lead:
                mask = 0.3 * randn(seed + 5, S, Tk)
                mask[:, :lead] = NINF
                mask[S - 1, lead - 1] = 0.0      # streams differ: the last one keeps one more key
            starts = None if ring is None else [(ring + s) % Tk for s in range(S)]
            kp, vp = (None, None) if ring is None else (kpos, vpos)
            st = starts or [0] * S
            want = _attention_ref(q.double(), k.double(), v.double(), st, None if kp is None else kp.double(), None if vp is None else vp.double(), mask, heads, causal)
            f32 = _attention_ref(q, k, v, st, kp, vp, mask, heads, causal)
            got = _attention_call(nat, dev, q, k, v, starts, kp, vp, mask, heads, hd, causal)
            bound = MARGIN * fp32_floor(f32, want)
            err = maxabs(got, want)
            worst = max(worst, err / bound)
            assert err <= bound, (S, shared, lead, ring, err, bound)
            if mask is not None:      # garbage in the masked keys' rows: bit for bit the clean result
                k2, v2 = k.clone(), v.clone()
                for s in range(S):
                    for j in range(Tk):
                        if mask[s, j] == NINF:
                            k2[s, (st[s] + j) % Tk] = 1e30
                            v2[s, (st[s] + j) % Tk] = 1e30
                again = _attention_call(nat, dev, q, k2, v2, starts, kp, vp, mask, heads, hd, causal)
                assert torch.equal(again, got), "a masked key leaked into the result"
    print(f"attention hd={hd} Tq={Tq} Tk={Tk} causal={causal}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------
# 2. the whole detector
# ------------------------------------------------------------------------------------------------
def _config(c):
    import streamformer_amd as sa
    return sa.OADConfig(VISUAL_SIZE=c["d_in"], NUM_CLASSES=c["classes"], LINEAR_ENABLED=c["linear_enabled"],
                        LINEAR_OUT_FEATURES=c["d_model"] if c["linear_enabled"] else -1, NUM_HEADS=c["heads"], DIM_FEEDFORWARD=c["ffn"],
                        ACTIVATION=c["activation"], LONG_MEMORY_NUM_SAMPLES=c["long_samples"], WORK_MEMORY_NUM_SAMPLES=c["work_samples"],
                        ENC_MODULE=c["enc_module"], DEC_MODULE=c["dec_module"])


def _detector(c, sd, mode):
    import streamformer_amd as sa
    det = sa.OnlineActionDetector(_config(c), compute_dtype=mode)
    res = det.load_state_dict(sd, strict=False)
    assert res.missing_keys == ["pos_encoding.pe"] and not res.unexpected_keys
    return det.to(gpu_device())


@functools.lru_cache(maxsize=None)
def _golden():
    return OO.load_golden()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sd, steps, fp64 oracle scores per step, {mode: floor scores per step}), computed once and shared."""
    sd, steps = OO.golden_case(_golden(), name)
    runs = {"want": OO.Stream(sd, OO.CASES[name])}
    for mode, bo in MODES.items():
        runs[mode] = OO.Stream(sd, OO.CASES[name], dtype=torch.float32, bf16_operands=bo)
    out = {k: [] for k in runs}
    for work, lg, mk, _ in steps:
        for k, st in runs.items():
            out[k].append(st.step(work, lg, mk))
    return sd, steps, out["want"], {m: out[m] for m in MODES}


def _bound(floor32, want):
    return MARGIN * fp32_floor(floor32, want)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(OO.CASES))
def test_detector_every_step_of_f20(name, mode):
    sd, steps, want, floors = _case(name)
    det = _detector(OO.CASES[name], sd, mode)
    state = det.new_state(1)
    worst = 0.0
    for t, (work, lg, mk, stored) in enumerate(steps):
        got = det.step(work, None if lg is None else [lg], mk, state=state)[0].cpu()
        bound = _bound(floors[mode][t], want[t])
        err = maxabs(got, want[t])
        worst = max(worst, err / bound)
        assert err <= bound, (t, err, bound)
        if mode == "fp32":
            assert maxabs(got, stored) <= bound, (t, maxabs(got, stored), bound)
    print(f"F20 {name} {mode}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(OO.CASES))
def test_ring_wrap_and_cached_memory(name, mode):
    sd, steps, want, floors = _case(name)
    c = OO.CASES[name]
    L = c["long_samples"]
    det = _detector(c, sd, mode)
    window = [r for r in steps[0][1]]
    last_long = None
    for t, (work, lg, mk, _) in enumerate(steps):
        if lg is not None and t:
            window = window[1:] + [lg[0]]
            last_long = t
    assert last_long is not None and sum(1 for s in steps[1:] if s[1] is not None) > L      # the ring has wrapped
    # a fresh state given the whole last window in one call agrees with the incremental one at the last step that pushed a sample
    inc = det.new_state(1)
    for t in range(last_long + 1):
        work, lg, mk, _ = steps[t]
        y_inc = det.step(work, None if lg is None else [lg], mk, state=inc)
    fresh = det.new_state(1)
    y_fresh = det.step(steps[last_long][0], [torch.stack(window)], steps[last_long][2], state=fresh)
    bound = _bound(floors[mode][last_long], want[last_long])
    assert maxabs(y_fresh, want[last_long]) <= bound and maxabs(y_inc, want[last_long]) <= bound
    assert maxabs(y_fresh, y_inc) <= bound
    # a call without a long sample reuses the cached compressed memory: bit-identical whatever state computed it, and repeatable
    work = steps[last_long + 1][0] if last_long + 1 < len(steps) else steps[0][0]
    a = det.step(work, None, None, state=inc)
    b = det.step(work, None, None, state=inc)
    assert torch.equal(a, b)
    twin = inc.clone()
    assert torch.equal(det.step(work, None, None, state=twin), a)


@pytest.mark.parametrize("mode", list(MODES))
def test_streams_are_independent(mode):
    name = "a"
    sd, steps, want, floors = _case(name)
    det = _detector(OO.CASES[name], sd, mode)
    fills = (0, 3, 8)                                  # steps already taken by streams 0, 1, 2
    together, alone = det.new_state(3), [det.new_state(1) for _ in fills]
    for s, n in enumerate(fills):
        for t in range(n):
            work, lg, mk, _ = steps[t]
            det.step(work, None if lg is None else [lg], mk, state=together, stream_ids=[s])
            det.step(work, None if lg is None else [lg], mk, state=alone[s])
    L = OO.CASES[name]["long_samples"]
    call = [steps[n] for n in fills]
    work = torch.stack([c[0] for c in call])
    longs = [c[1] for c in call]
    mask = torch.stack([c[2] if c[2] is not None else torch.zeros(L, dtype=torch.float64) for c in call])
    twin = together.clone()
    y = det.step(work, longs, mask, state=together).cpu()
    assert torch.equal(det.step(work, longs, mask, state=twin).cpu(), y), "the same call on a cloned state differs"
    for s, n in enumerate(fills):
        single = det.step(call[s][0], None if call[s][1] is None else [call[s][1]], call[s][2], state=alone[s])[0].cpu()
        bound = _bound(floors[mode][n], want[n])
        assert maxabs(y[s], want[n]) <= bound and maxabs(single, want[n]) <= bound, (s, maxabs(y[s], want[n]), bound)
        assert maxabs(y[s], single) <= bound
    # reset of stream 1: it equals a fresh stream, its neighbours are untouched
    together.reset(1)
    assert together.fill(1) == 0 and together.fill(0) == L and together.fill(2) == L
    fresh = det.new_state(1)
    w0, l0, m0, _ = steps[0]
    w3 = torch.stack([steps[fills[0] + 1][0], w0, steps[fills[2] + 1][0]])
    l3 = [steps[fills[0] + 1][1], l0, steps[fills[2] + 1][1]]
    m3 = torch.stack([torch.zeros(L, dtype=torch.float64) if s[2] is None else s[2] for s in (steps[fills[0] + 1], steps[0], steps[fills[2] + 1])])
    after = det.step(w3, l3, m3, state=together).cpu()
    assert torch.equal(after[1], det.step(w0, [l0], m0, state=fresh)[0].cpu()), "a reset stream differs from a fresh one"
    untouched = det.step(w3[[0, 2]], [l3[0], l3[2]], m3[[0, 2]], state=twin, stream_ids=[0, 2]).cpu()
    assert torch.equal(after[[0, 2]], untouched), "reset(1) changed a neighbour"


def test_full_width_case():
    """d_in 768, d_model 1024, 4 heads of 256, FFN 1024, L 64, W 32, Q0 16, 22 classes: 3 steps of one stream, the second pushes a sample."""
    c = OO.FULL
    sd = OO.make_weights(c, 2003)
    L, W = c["long_samples"], c["work_samples"]
    window, work, new = randn(1, L, c["d_in"]), randn(2, 3, W, c["d_in"]), randn(3, 1, c["d_in"])
    mask = torch.zeros(L)
    mask[:5] = NINF
    plan = [(work[0], window, mask), (work[1], new, mask), (work[2], None, None)]
    runs = {"want": OO.Stream(sd, c)}
    for mode, bo in MODES.items():
        runs[mode] = OO.Stream(sd, c, dtype=torch.float32, bf16_operands=bo)
    ref = {k: [st.step(w, lg, mk) for w, lg, mk in plan] for k, st in runs.items()}
    for mode in MODES:
        det = _detector(c, sd, mode)
        state = det.new_state(1)
        for t, (w, lg, mk) in enumerate(plan):
            got = det.step(w, None if lg is None else [lg], mk, state=state)[0].cpu()
            bound = _bound(ref[mode][t], ref["want"][t])
            err = maxabs(got, ref["want"][t])
            print(f"full width {mode} step {t}: error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (mode, t, err, bound)


def _reference_long_plan(frames_total, L, W, rate):
    """The reference's loop (engines/lstr/lstr_inference.py:69-99) restated on frame indices alone: for every step work_start = 0, 1, ...
    (work window [work_start, work_start + W)) -> (long frame indices passed or None, masked leading slots)."""
    from bisect import bisect_right
    plan, long_indices = [], None
    for work_start in range(frames_total - W + 1):
        long_end = work_start - 1
        if long_end == -1:
            long_indices = [0 for _ in range(L)]
            passed = list(long_indices)
        elif long_end % rate == 0:
            long_indices = long_indices[1:] + [long_end]
            passed = [long_end]
        else:
            passed = None
        last_zero = bisect_right(long_indices, 0) - 1
        plan.append((passed, max(last_zero, 0)))
    return plan


def test_streaming_action_detector():
    import streamformer_amd as sa
    from streamformer_amd.init_weights import make_state_dict
    dev = gpu_device()
    cfg = small_cfg()
    tower = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype="fp32")
    tower.load_state_dict(make_state_dict(cfg, seed=4))
    tower = tower.to(dev).eval()
    c = dict(OO.CASES["b"], d_in=cfg.hidden_size, d_model=cfg.hidden_size, long_samples=4, work_samples=3)
    det = _detector(c, OO.make_weights(c, 2004), "fp32")
    L, W, rate, T = 4, 3, 2, 12
    assert [m for _, m in _reference_long_plan(T, L, W, rate)][:8] == [3, 3, 3, 2, 2, 1, 1, 0]      # frame 0 pushed again at step 1: still 3 masked
    plan = _reference_long_plan(T, L, W, rate)
    sad = sa.StreamingActionDetector(tower, det, long_sample_rate=rate)
    x = frames(11, (T, 3, cfg.image_size, cfg.image_size))
    state = det.new_state(1)
    feats = []
    for t in range(T):
        p = sad.push(x[t])
        assert p.shape == (c["classes"],) and torch.isfinite(p).all() and abs(float(p.sum()) - 1.0) < 1e-5
        feats.append(sad.last_features.clone())
        # the reference starts at the first full work window (step 0 = push W - 1); before it the stream is younger than W frames: the
        # window is padded with frame 0 (the data layer's clip(0)) and the long window is the initial one, passed at push 0
        if t == 0:
            passed, masked = [0] * L, L - 1
        elif t < W - 1:
            passed, masked = None, None
        elif t == W - 1:
            passed, masked = None, None                       # step 0's window was passed at push 0 already, with the same mask
            assert plan[0] == ([0] * L, L - 1)
        else:
            passed, masked = plan[t - W + 1]
        long = mask = None
        if passed is not None:
            long = torch.stack([feats[j] for j in passed])
            mask = torch.zeros(L)
            mask[:masked] = NINF
        work = torch.stack([feats[max(0, j)] for j in range(t - W + 1, t + 1)])
        by_hand = det.step(work, None if long is None else [long], mask, state=state, probs=True)[0, -1]
        assert torch.equal(by_hand, p), t
    assert plan[-1][1] == 0 and sad.long_indices == [j for j in range(T - W) if j % rate == 0][-L:]
