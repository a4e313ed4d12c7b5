"""The single backward operators of the training step — sf_op_attention_bwd, sf_op_attention_bwd_hd, sf_op_layernorm_bwd, sf_op_wgrad —
against fp64 restatements on identical inputs (tests/backward_oracle.py), at every tile edge of the kernels and inside guard rows.

Bounds follow tests/test_oad.py and tests/test_msda.py: every bound is MARGIN = 4 times a PRECISION FLOOR that is computed here, on the
CPU, from the inputs — the same metric for the reference operator sequence in fp32 against its fp64 run — and never from the code under
test.  Small attention cases have a floor of exactly 0 (no bf16 value lands on the other side of a rounding boundary in the fp32 run), so
the floor of a metric is the largest over the cases of its kernel FAMILY: tuned spatial, tuned temporal, generic spatial, generic
temporal, LayerNorm backward per MAXV instance (and input regime), weight gradient.  The attention floors take the fp32 run in ORDERS = 8
summation orders on the same inputs (_attn_case says why).  The fp32 outputs (LayerNorm, weight gradient) have a floor of at least one
fp32 rounding of the result, as in test_msda.py.  ONE exception to "MARGIN x a floor": at L = 1 dq and dk are exactly 0, a relative
metric does not exist, and _check_zero_slices bounds the values by the cancellation residue of two fp32 dot products instead.

Attention backward is compared with an OPERAND-MATCHED reference: fp64 with a bf16 rounding wherever the kernel makes one (listed in
backward_oracle.attention_backward), per slice (dq, dk, dv) in two metrics — (a) relative L2, (b) the worst token row of one head over
the slice's RMS row norm.  One loose check against the exact fp64 gradient (bound: MARGIN x the matched reference's own distance from it,
the bf16 rounding of the results) keeps a mistake in the emulation from hiding one in the kernel.  test_metrics_catch_a_wrong_ds is the
CPU-side evidence that these bounds are tight enough to see a 1 % error in dS, a lost query row or a half-weighted key.

The edge of this work: the pooling-head backward, the GELU backward and the gate / head-query gradients have no single-operator entry;
they stay covered by the whole-model gradient tests of test_train_parity.py and test_train_widths.py.

The largest error / bound ratio measured on the MI355X stands next to each family's case list below and in DESIGN.md (training section);
against the exact fp64 gradient it is 0.25 in every attention family: the kernels' distance from it IS the bf16 rounding of the results.
"""
import functools
import zlib

import pytest
import torch

from tests import backward_oracle as BO
from tests.helpers import EPS32, MARGIN, gpu_device

gpu = pytest.mark.gpu

ORDERS = 8                # summation orders of the fp32 run that a floor is taken over (_attn_case)
GUARD_ROWS = 64
NAN16 = 0x7FC5            # quiet bf16 NaN with a payload, compared as int16
NAN32 = 0x7FC00A5A        # the same for fp32 buffers, compared as int32
SLICES = ("dq", "dk", "dv")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _report(what, err, bound):
    print(f"  [backward precision] {what}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound if bound > 0 else float(err > 0):.3f}")
    return err <= bound


# ---------------------------------------------------------------------------------------------------
# attention backward: cases
# ---------------------------------------------------------------------------------------------------
# key = (layout, B, N, heads, hd, L, causal, input scale); spatial: B frames, N = 1
# tuned spatial: 16- and 32-token tiles, the compile-time 13-tile instance (193..208), the last tile (209..224)
# largest ratio vs matched: rel-L2 0.24, worst row 0.25 (dv, L 191)
SPATIAL_L = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 191, 192, 193, 196, 207, 208, 209, 223, 224)
TUNED_SPATIAL = [(0, 3, 1, 3, 64, L, 0, 1.5) for L in SPATIAL_L] + [(0, 3, 1, 3, 64, L, 0, s) for L in (196, 224) for s in (3.0, 0.25)]
# tuned temporal: 16- and 32-row images, 10 and 9 wave-sized problems on 4-wave workgroups (a partly filled one next to full ones)
# largest ratio vs matched: rel-L2 0.06 (dk, (1, 3, 3), L 2, causal), worst row 0.06 (dq, (2, 5, 1), L 31, causal)
TEMPORAL_L = (1, 2, 3, 4, 8, 15, 16, 17, 24, 31, 32)
TUNED_TEMPORAL = [(1, B, N, h, 64, L, c, 1.5) for (B, N, h) in ((2, 5, 1), (1, 3, 3)) for L in TEMPORAL_L for c in (1, 0)]
# generic kernel: lanes over keys, 64 per wave
# largest ratio vs matched: spatial rel-L2 0.17 (dq, hd 72, L 64), worst row 0.17 (dq, hd 72, L 196); temporal rel-L2 0.28, worst row 0.25
# (dv, hd 128, L 32, causal).  At one summation order the temporal floor was 3.0e-5 and dq at hd 72, L 17, causal stood at 1.41 of its bound:
# ONE result on the other side of a bf16 boundary, the same one that other summation orders of the fp32 emulation move (_attn_case)
GENERIC_SPATIAL = [(0, 2, 1, 2, hd, L, 0, 1.5) for hd in (8, 72, 128) for L in (1, 63, 64, 65, 196, 224)]
GENERIC_TEMPORAL = [(1, 2, 3, 2, hd, L, c, 1.5) for hd in (8, 72, 128) for L in (1, 17, 32) for c in (1, 0)]
FAMILIES = {"tuned spatial": TUNED_SPATIAL, "tuned temporal": TUNED_TEMPORAL, "generic spatial": GENERIC_SPATIAL,
            "generic temporal": GENERIC_TEMPORAL}


def _mode(key):
    return "tuned" if key[4] == 64 else "generic"


def _slices(L):
    """the slices that have relative metrics: at L = 1 dS = P (dP - Delta) is identically 0, so dq and dk are too (_check_zero_slices)"""
    return [(i, name) for i, name in enumerate(SLICES) if L > 1 or name == "dv"]


def _metrics(got, want, heads, hd):
    """{(slice, metric): value} of a [nseq, L, 3D] result against a reference"""
    D = heads * hd
    out = {}
    for i, name in _slices(got.shape[1]):
        g, w = got[..., i * D:(i + 1) * D], want[..., i * D:(i + 1) * D]
        out[name, "rel-L2"] = BO.rel_l2(g, w)
        out[name, "worst row"] = BO.worst_row(g, w, heads, hd)
    return out


@functools.lru_cache(maxsize=None)
def _attn_case(key):
    """inputs (sequence form, distinct data per sequence and head), the two fp64 references and the case's own floors; computed once"""
    layout, B, N, heads, hd, L, causal, scale = key
    nseq, D = B * N, heads * hd
    g = _gen("attention", key)
    qkv = (torch.randn(nseq, L, 3 * D, generator=g) * scale).bfloat16()
    d_o = torch.randn(nseq, L, D, generator=g).bfloat16()
    o = BO.attention_forward(qkv, heads, hd, bool(causal)).bfloat16()
    args = (qkv, o, d_o, heads, hd, bool(causal))
    exact = BO.attention_backward(*args, mode="exact")
    matched = BO.attention_backward(*args, mode=_mode(key))
    # The floor: the fp32 run of the matched emulation against its fp64 run, the largest over ORDERS summation orders of the fp32 run
    # on these same inputs (backward_oracle.attention_backward, `order`).  What separates any fp32 implementation from the fp64 emulation
    # is which results that sit next to a bf16 rounding boundary land on the other side; the inputs decide which results sit there, the
    # summation order decides which of them move.  One order samples that once; in a slice of a few thousand elements a single moved
    # element IS the metric, so one sample says little.  The pooled figures stop moving at 8 orders (8 -> 16: at most 1.3 x).
    floor = {}
    for order in range(ORDERS):
        f32 = BO.attention_backward(*args, dtype=torch.float32, mode=_mode(key), order=order if order else None)
        for k, v in _metrics(f32, matched, heads, hd).items():
            floor[k] = max(floor.get(k, 0.0), v)
    return dict(qkv=qkv, o=o, d_o=d_o, exact=exact, matched=matched, floor=floor,
                exact_floor={n: BO.rel_l2(matched[..., i * D:(i + 1) * D], exact[..., i * D:(i + 1) * D]) for i, n in _slices(L)})


@functools.lru_cache(maxsize=None)
def _attn_floor(family):
    """{(slice, metric): largest floor over the family's cases}"""
    pooled = {}
    for key in FAMILIES[family]:
        for k, v in _attn_case(key)["floor"].items():
            pooled[k] = max(pooled.get(k, 0.0), v)
    assert len(pooled) == 6 and all(v > 0 for v in pooled.values()), (family, pooled)
    return pooled


def _check_zero_slices(got, key):
    """L = 1: P = 1 and dP = Delta = dO . V, so dq = dk = 0.  The kernels form dP and Delta as two fp32 dot products of length head_dim
    in different orders; each is within head_dim * 2^-24 * sum |dO_e V_e| of the exact value (the standard bound of a dot product in any
    order), the residue goes through scale, one bf16 rounding of dS (tuned kernels), the factor k or q and the bf16 rounding of the
    result (together < 1 + 2^-6).  A bound from the number formats alone: no floor, no MARGIN."""
    layout, B, N, heads, hd, L, causal, _ = key
    c = _attn_case(key)
    D = heads * hd
    q, k, v = (c["qkv"][..., i * D:(i + 1) * D].double().reshape(-1, heads, hd) for i in range(3))
    g = c["d_o"].double().reshape(-1, heads, hd)
    residue = 2 * hd * EPS32 * (g * v).abs().sum(-1, keepdim=True) * hd ** -0.5 * (1 + 2.0 ** -6)
    for i, other in ((0, k), (1, q)):
        err = got[..., i * D:(i + 1) * D].double().reshape(-1, heads, hd).abs()
        bound = residue * other.abs()
        worst = float((err / (bound + 1e-300)).max())
        print(f"  [backward precision] {key} {SLICES[i]} (exactly 0): largest |value| {float(err.max()):.3e}, {worst:.3f} of the cancellation bound")
        assert bool((err <= bound).all()), (key, SLICES[i])


def _guarded(dev, rows, width, dtype):
    """A buffer of `rows` rows with GUARD_ROWS rows in front and behind, every element one non-finite bit pattern:
    (whole buffer as integers, interior view in `dtype`, interior view as integers, the pattern)"""
    if dtype == torch.bfloat16:
        ints = torch.full((rows + 2 * GUARD_ROWS, width), NAN16, dtype=torch.int16, device=dev)
        pattern = NAN16
    else:
        ints = torch.full((rows + 2 * GUARD_ROWS, width), NAN32, dtype=torch.int32, device=dev)
        pattern = NAN32
    inner = ints[GUARD_ROWS:GUARD_ROWS + rows]
    return ints, inner.view(dtype), inner, pattern


def _check_guards(ints, inner_ints, pattern, what):
    rows = inner_ints.shape[0]
    assert bool((ints[:GUARD_ROWS] == pattern).all()), f"{what}: wrote in front of the tensor"
    assert bool((ints[GUARD_ROWS + rows:] == pattern).all()), f"{what}: wrote behind the tensor"
    assert not bool((inner_ints == pattern).any()), f"{what}: elements of the tensor left unwritten"


def _run_attention(key, fn="auto"):
    """d_qkv of the case on the GPU, in sequence form on the CPU (bf16); guard rows checked"""
    import streamformer_amd._native as nat
    dev = gpu_device(or_skip=True)
    layout, B, N, heads, hd, L, causal, _ = key
    c = _attn_case(key)
    nseq, D = B * N, heads * hd
    if fn == "auto":
        fn = "sf_op_attention_bwd" if hd == 64 else "sf_op_attention_bwd_hd"

    def tokens(t):       # sequence form -> the kernel's token rows
        return (BO.from_sequences(t, B, N) if layout == 1 else t).reshape(nseq * L, -1).contiguous().to(dev)
    qd, od, dod = tokens(c["qkv"]), tokens(c["o"]), tokens(c["d_o"])
    ints, dq, dq_ints, pattern = _guarded(dev, nseq * L, 3 * D, torch.bfloat16)
    args = [qd.data_ptr(), od.data_ptr(), dod.data_ptr(), dq.data_ptr(), layout, nseq, L, N, heads]
    args += [hd, causal] if fn == "sf_op_attention_bwd_hd" else [causal]
    nat.check(getattr(nat.lib, fn)(*args, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    _check_guards(ints, dq_ints, pattern, f"d_qkv {key}")
    out = dq.cpu()
    assert bool(torch.isfinite(out.float()).all()), key
    return BO.to_sequences(out.reshape(B, L, N, 3 * D)) if layout == 1 else out.reshape(nseq, L, 3 * D)


def _check_attention(family, key):
    layout, B, N, heads, hd, L, causal, _ = key
    gpu_device(or_skip=True)
    c, bound = _attn_case(key), {k: MARGIN * v for k, v in _attn_floor(family).items()}
    got = _run_attention(key)
    again = _run_attention(key)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "not bit-reproducible"
    ok = True
    for (name, metric), err in _metrics(got, c["matched"], heads, hd).items():
        ok &= _report(f"{family} {key} {name} {metric} vs matched", err, bound[name, metric])
    D = heads * hd
    for i, name in _slices(L):
        err = BO.rel_l2(got[..., i * D:(i + 1) * D], c["exact"][..., i * D:(i + 1) * D])
        ok &= _report(f"{family} {key} {name} rel-L2 vs exact", err, MARGIN * c["exact_floor"][name])
    if L == 1:
        _check_zero_slices(got, key)
    assert ok, (family, key)


@gpu
@pytest.mark.parametrize("key", TUNED_SPATIAL, ids=lambda k: f"L{k[5]}-x{k[7]}")
def test_tuned_spatial_attention_bwd(key):
    _check_attention("tuned spatial", key)


@gpu
@pytest.mark.parametrize("key", TUNED_TEMPORAL, ids=lambda k: f"B{k[1]}-N{k[2]}-h{k[3]}-L{k[5]}-c{k[6]}")
def test_tuned_temporal_attention_bwd(key):
    _check_attention("tuned temporal", key)


@gpu
@pytest.mark.parametrize("key", GENERIC_SPATIAL, ids=lambda k: f"hd{k[4]}-L{k[5]}")
def test_generic_spatial_attention_bwd(key):
    _check_attention("generic spatial", key)


@gpu
@pytest.mark.parametrize("key", GENERIC_TEMPORAL, ids=lambda k: f"hd{k[4]}-L{k[5]}-c{k[6]}")
def test_generic_temporal_attention_bwd(key):
    _check_attention("generic temporal", key)


@gpu
@pytest.mark.parametrize("key", [(0, 3, 1, 3, 64, 17, 0, 1.5), (1, 2, 5, 1, 64, 31, 1, 1.5)], ids=["spatial-L17", "temporal-L31"])
def test_head_dim_64_entry_stays_the_tuned_kernel_at_the_new_edges(key):
    gpu_device(or_skip=True)
    a = _run_attention(key, fn="sf_op_attention_bwd_hd")
    b = _run_attention(key, fn="sf_op_attention_bwd")
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------------
# the metrics can fail (CPU only: emulation against emulation, no kernel)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,key", [("tuned spatial", (0, 3, 1, 3, 64, 193, 0, 1.5)), ("tuned temporal", (1, 2, 5, 1, 64, 17, 1, 1.5))],
                         ids=["spatial-L193", "temporal-causal-L17"])
def test_metrics_catch_a_wrong_ds(family, key):
    """dS scaled by 1.01, the last query row dropped from dS, the last key's dS column halved: each must exceed MARGIN x the family's
    pooled floor in metric (a) or (b), and the ordinary fp32 run must stay within it."""
    assert key in FAMILIES[family]
    heads, hd, causal = key[3], key[4], key[6]
    c, bound = _attn_case(key), {k: MARGIN * v for k, v in _attn_floor(family).items()}
    for k, v in c["floor"].items():
        assert _report(f"{family} {key} fp32 run {k}", v, bound[k])
    for fault in BO.FAULTS:
        wrong = BO.attention_backward(c["qkv"], c["o"], c["d_o"], heads, hd, bool(causal), mode="tuned", fault=fault)
        m = _metrics(wrong, c["matched"], heads, hd)
        worst = max(m, key=lambda k: m[k] / bound[k])
        print(f"  [backward precision] {family} {key} {fault}: {worst} {m[worst]:.3e} = {m[worst] / bound[worst]:.1f} x bound")
        assert m[worst] > bound[worst], (fault, m, bound)


# ---------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------
LN_EPS = 1e-6
# key = (rows, D, regime, g_in given, d_gamma / d_beta given).  sf_launch_ln_bwd: MAXV 1 for D <= 256, 3 for D <= 768, 8 for D <= 2048;
# the finish kernel takes 64 columns per block; rows > 2048 enter the grid-stride loop
# largest ratio: standard inputs 0.25 (dx, MAXV 1) / 0.21 (MAXV 3) / 0.20 (MAXV 8); mean 30 +- 0.5: 0.40 (d_beta, D 768), 0.71 (d_gamma, D 1152);
# rstd decided by eps: 0.22 (d_gamma, D 768), 0.23 (d_beta, D 1152)
LN_CASES = ([(37, D, "standard", True, True) for D in (4, 64, 68, 252, 256, 260, 576, 768, 772, 1024, 1152, 2048)]
            + [(rows, D, "standard", True, True) for rows in (1, 5, 2048, 2049, 4100) for D in (64, 768, 1152)]
            + [(37, D, regime, True, True) for D in (768, 1152) for regime in ("cancellation", "eps decides")]
            + [(37, D, "standard", False, True) for D in (64, 768, 1152)]
            + [(37, D, "standard", True, False) for D in (64, 768, 1152)])


def _ln_family(key):
    D, regime = key[1], key[2]
    return (1 if D <= 256 else 3 if D <= 768 else 8, regime)


@functools.lru_cache(maxsize=None)
def _ln_case(key):
    rows, D, regime, with_gin, with_dgdb = key
    g = _gen("layernorm", key)
    if regime == "standard":
        x = torch.randn(rows, D, generator=g) * 2 + 0.3
    elif regime == "cancellation":          # variance by cancellation: mean 30, deviation 0.5
        x = 30 + 0.5 * torch.randn(rows, D, generator=g)
    else:                                   # rstd decided by eps: one exactly constant row, one row of deviation 1e-3.  The constant is
        x = torch.randn(rows, D, generator=g) * 2 + 0.3      # 1.5: every partial sum of D <= 2048 copies is exact in fp32, so the row
        x[11] = 1.5                                          # centres to exactly 0 in any summation order (variance 0, rstd = eps^-1/2)
        x[23] = 0.7 + 1e-3 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    gamma = torch.randn(D, generator=g)
    g_in = torch.randn(rows, D, generator=g) if with_gin else None
    base_g, base_b = torch.randn(D, generator=g), torch.randn(D, generator=g)      # d_gamma / d_beta accumulate onto these
    want = BO.layernorm_backward(x, dy, gamma, g_in, LN_EPS)
    want = (want[0], base_g.double() + want[1], base_b.double() + want[2])
    f32 = BO.layernorm_backward(x, dy, gamma, g_in, LN_EPS, dtype=torch.float32)
    f32 = (f32[0], base_g + f32[1], base_b + f32[2])
    floor = {n: max(BO.rel_max(f, w), EPS32) for n, f, w in zip(("dx", "d_gamma", "d_beta"), f32, want)}
    return dict(x=x, dy=dy, gamma=gamma, g_in=g_in, base_g=base_g, base_b=base_b, want=want, floor=floor)


@functools.lru_cache(maxsize=None)
def _ln_floor(family):
    pooled = {}
    for key in LN_CASES:
        if _ln_family(key) == family:
            for k, v in _ln_case(key)["floor"].items():
                pooled[k] = max(pooled.get(k, 0.0), v)
    return pooled


@gpu
@pytest.mark.parametrize("key", LN_CASES, ids=lambda k: f"rows{k[0]}-D{k[1]}-{k[2].replace(' ', '_')}-gin{int(k[3])}-dgdb{int(k[4])}")
def test_layernorm_bwd(key):
    dev = gpu_device(or_skip=True)
    import streamformer_amd._native as nat
    rows, D, regime, with_gin, with_dgdb = key
    c, floor = _ln_case(key), _ln_floor(_ln_family(key))
    xd, dyd, gd = c["x"].to(dev), c["dy"].to(dev), c["gamma"].to(dev)
    gind = c["g_in"].to(dev) if with_gin else None
    dg, db = c["base_g"].to(dev), c["base_b"].to(dev)
    ints, dx, dx_ints, pattern = _guarded(dev, rows, D, torch.float32)
    nat.check(nat.lib.sf_op_layernorm_bwd(xd.data_ptr(), dyd.data_ptr(), gd.data_ptr(), gind.data_ptr() if with_gin else 0, dx.data_ptr(),
                                          dg.data_ptr() if with_dgdb else 0, db.data_ptr() if with_dgdb else 0, rows, D, LN_EPS,
                                          nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    _check_guards(ints, dx_ints, pattern, f"dx {key}")
    fam = "LayerNorm MAXV %d %s" % _ln_family(key)
    ok = _report(f"{fam} {key} dx", BO.rel_max(dx.cpu(), c["want"][0]), MARGIN * floor["dx"])
    if with_dgdb:
        ok &= _report(f"{fam} {key} d_gamma", BO.rel_max(dg.cpu(), c["want"][1]), MARGIN * floor["d_gamma"])
        ok &= _report(f"{fam} {key} d_beta", BO.rel_max(db.cpu(), c["want"][2]), MARGIN * floor["d_beta"])
    else:      # no column sums asked for: the buffers the launcher was not given stay as they were
        assert torch.equal(dg.cpu(), c["base_g"]) and torch.equal(db.cpu(), c["base_b"])
    assert ok, key


# ---------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------
# key = (M, N1, N2, accumulate).  sf_launch_wgrad needs ldy % 8, ldx % 8, N2 % 4, ldo % 4 (and the bias column sums N1 % 8); 64 token rows
# per K-step in two 32-row MFMA steps: M = 1, one row short of / past one 32-row step, one row past 64 K-steps
# largest ratio: out 0.04, d_bias 0.15 (both at M 4097)
WGRAD_CASES = [(M, N1, N2, acc) for M in (1, 31, 33, 4097) for (N1, N2) in ((72, 200), (64, 64)) for acc in (0, 1)]
WGRAD_ALPHA = 0.5
WGRAD_PAD = 8
SENTINEL = -123456.0


@functools.lru_cache(maxsize=None)
def _wgrad_case(key):
    M, N1, N2, acc = key
    g = _gen("wgrad", key)
    dy = torch.randn(M, N1, generator=g).bfloat16()
    x = torch.randn(M, N2, generator=g).bfloat16()
    base = torch.randn(N1, N2, generator=g)
    base_b = torch.randn(N1, generator=g)
    want = WGRAD_ALPHA * BO.wgrad(dy, x) + (base.double() if acc else 0)
    f32 = WGRAD_ALPHA * BO.wgrad(dy, x, torch.float32) + (base if acc else 0)
    want_b = base_b.double() + WGRAD_ALPHA * dy.double().sum(0)          # the bias gradient always accumulates
    f32_b = base_b + WGRAD_ALPHA * dy.float().sum(0)
    floor = {"out": max(BO.rel_max(f32, want), EPS32), "d_bias": max(BO.rel_max(f32_b, want_b), EPS32)}
    return dict(dy=dy, x=x, base=base, base_b=base_b, want=want, want_b=want_b, floor=floor)


@functools.lru_cache(maxsize=None)
def _wgrad_floor():
    return {k: max(_wgrad_case(key)["floor"][k] for key in WGRAD_CASES) for k in ("out", "d_bias")}


@gpu
@pytest.mark.parametrize("key", WGRAD_CASES, ids=lambda k: f"M{k[0]}-{k[1]}x{k[2]}-acc{k[3]}")
def test_wgrad(key):
    dev = gpu_device(or_skip=True)
    import streamformer_amd._native as nat
    M, N1, N2, acc = key
    c, floor = _wgrad_case(key), _wgrad_floor()
    ldo = N2 + WGRAD_PAD
    ints, out, out_ints, pattern = _guarded(dev, N1, ldo, torch.float32)
    out[:, N2:] = SENTINEL
    if acc:
        out[:, :N2] = c["base"].to(dev)
    dyd, xd, db = c["dy"].to(dev), c["x"].to(dev), c["base_b"].to(dev)
    nat.check(nat.lib.sf_op_wgrad(dyd.data_ptr(), N1, xd.data_ptr(), N2, M, N1, N2, WGRAD_ALPHA, acc, out.data_ptr(), ldo, db.data_ptr(),
                                  nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    _check_guards(ints, out_ints[:, :N2], pattern, f"wgrad {key}")
    assert bool((out[:, N2:] == SENTINEL).all()), "wrote into the columns between N2 and ldo"
    ok = _report(f"wgrad {key} out", BO.rel_max(out[:, :N2].cpu(), c["want"]), MARGIN * floor["out"])
    ok &= _report(f"wgrad {key} d_bias", BO.rel_max(db.cpu(), c["want_b"]), MARGIN * floor["d_bias"])
    assert ok, key
