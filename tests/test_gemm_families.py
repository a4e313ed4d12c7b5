"""GPU: every forward GEMM family (skinny, tile, panel, 256^2, 128^2) and every epilogue ALONE, through sf_op_gemm, against fp64 of the
same operand planes (tests/gemm_oracle.py).

Bounds (tests/helpers.py): MARGIN = 4 times what the floor model — the same expression in fp32, computed on the CPU from the inputs —
loses against fp64, never less than EPS32 max|want|.  A bf16 output may additionally be off by half a bf16 ulp of the fp64 value; two
planes hold the value to 2^-17 relative, three to 2^-25, plus the floor; the hi plane is a nearest bf16 number to hi + lo (+ lo2)
(``is_nearest_bf16``: bf16_round of it, except where the planes' sum is an exact tie) and |lo| <= half an ulp of hi.

Every output, plane and statistics buffer has a pitch of N + 8, NaN (fp32) or a NaN bit pattern (bf16) in the pad columns, in the rows
a remap does not name and in a guard row behind it; statistics buffers are cleared as the forward clears them (zeros where the layout
writes nothing) and NaN where a pair must be written.  Every case names its family or asserts ``family_taken``.

Largest error / bound per group on an MI355X, as the run prints it with ``-s`` (whole file: 24 s wall, 99 tests; also DESIGN.md 1.2):

    group                                   128^2          skinny         tile (auto; ids 0 .. 5)          panel   256^2
                                            bf16   bf16x3  bf16   bf16x3  bf16                             bf16    bf16    bf16x3
    F32                                     0.35   0.38    0.60   0.73    0.34; 0.36 0.34 0.34 - - -       0.22    0.41    0.57
    RESID (fp32 residual)                   0.35   0.31    0.45   0.67    0.32; 0.23 0.22 0.23 - - -       0.21    0.34    0.48
    RESID, K = 768 unrolled                 -      -       0.18   -       -                                -       -       -
    RESID with resid_mod                    -      -       -      -       -                                0.23    -       -
    EMBED                                   0.30   0.32    0.47   0.81    0.27; 0.24 0.24 0.27 - - -       -       -       -
    BF16 (bf16x3: hi + lo)                  1.000  0.94    1.000  0.93    1.000; 1.000 on every id         1.000   1.000   0.88
    ACT_BF16                                1.000  0.91    1.000  0.89    1.000; 0.999 0.999 1.000 1.000 0.999 0.999   -   0.98  0.89
    fold in kernel  BF16 / ACT / F32        -      -       0.990 / 0.990 / -;  bf16x3 0.31 / 0.23 / 0.30
                                                                          0.999 / 0.971; id 3 0.994 / 0.968, id 4 0.994 / 0.969
    fold consumer (statistics)  BF16 / ACT  -      -       -      -       -                                -       0.992 / 0.969   0.279 / 0.282
    RESID + statistics, fp32 rows + hi      -      -       -      -       value 0.25, sum x 0.20, sum x^2 0.28 (EMBED: 0.26, 0.21, 0.29)
    RESID planes + statistics               -      -       -      -       -       value 0.94, sum x 0.12, sum x^2 0.13 (panel)
                                                                                  0.93, 0.14, 0.13 (256^2 bf16);  0.43, 0.15, 0.15 (256^2 bf16x3)

    256^2 row tiles, bf16x3, forced 160 / 192 / 224 / 256 and without 224: F32 0.25, planes 0.29, sum x 0.13, sum x^2 0.14 on each
    256^2 row tiles, bf16, without 224 (256-row tiles): F32 0.20, BF16 1.000, ACT 0.97, planes 0.92 / 0.15 / 0.13, fold consumer BF16 0.990, ACT 0.972
    column split through dispatch: bf16x3 F32 0.29, RESID 0.28; bf16 F32 0.21, BF16 1.000; (2049, 1152, 128) in bf16 (skinny): 0.23
    chains (reference: fp64 LayerNorm then Linear, exact operands), BF16 / ACT_BF16:
      panel -> 256^2 bf16 0.246 / 0.254;  256^2 -> 256^2 bf16 0.250 / 0.245, bf16x3 0.249 / 0.243;  tile (statistics) -> 256^2 0.258 / 0.243
      tile -> tile (in kernel) 0.250 / 0.236;  skinny -> skinny (in kernel) bf16 0.263 / 0.245, bf16x3 0.255 / 0.243

  * 1.000 (0.99 and up) on every ONE-plane bf16 output is the bound doing its work, not a kernel at its limit: the bound is half a bf16
    ulp of the fp64 value plus four floors, the floor is 2^-16 of that ulp, and a correctly rounded output is off by up to exactly half
    an ulp.  A kernel that rounded twice, truncated, or took its value one column over would exceed it ("Seeing a fault").
  * The chains sit at 1 / MARGIN = 0.25: against a reference with exact operands the error IS the operand rounding (and, on the rows
    of mean 8, the cancellation behind it), the fp32 floor model makes the same roundings as the kernels, and so error = floor.
  * Nothing is below 0.01.  The lowest, the statistics at 0.12 .. 0.29, are sums of 192 .. 384 fp32 values against a floor that adds
    them one chunk after the other (``_chunked_sum``) and a rounding of their terms (next point); the kernels' tree reductions lose less.
  * Statistics: sum x and sum x^2 have bounds of their own, and the rounding below which neither goes is that of the sum's TERMS,
    EPS32 sum |term| (never more than EPS32 max|statistics row|, which is what one check over the whole buffer would use).  With
    EPS32 |sum x| instead, the tile producers at M = 1 (one row, sum x = 9.0 and 2.9 out of sum |x| = 237 and 213) measured 2.39 (RESID)
    and 1.62 (EMBED): the kernel's 5.1e-6 is 3.9e-6 of fp32 summation of its own, correct rows plus 1.2e-6 of their roundings, and the
    fp32 floor model misses that limit itself on a fifth of all rows (test_gemm_oracle_cpu.py).
"""
import ctypes as C

import pytest
import torch

from tests import gemm_oracle as G
from tests.helpers import EPS32, MARGIN, gpu_device, maxabs, randn

pytestmark = pytest.mark.gpu

AUTO, SKINNY, TILE, PANEL, G256, G128, COLSPLIT = range(7)
FAMILY = {SKINNY: "skinny", TILE: "tile", PANEL: "panel", G256: "256^2", G128: "128^2", COLSPLIT: "colsplit"}
EPI = {G.F32: "F32", G.BF16: "BF16", G.ACT_BF16: "ACT_BF16", G.RESID_F32: "RESID", G.EMBED_F32: "EMBED"}
NAN16 = 0x7FC1          # a bf16 NaN no kernel produces: the fill of bf16 buffers
PAD = 8
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    print("\n  largest error / bound per family | mode | epilogue group:")
    for k in sorted(RATIOS):
        print(f"    {k:58s} {RATIOS[k][0]:.3f}   ({RATIOS[k][1]} cases)")


def note(group, ratio):
    r, n = RATIOS.get(group, (0.0, 0))
    RATIOS[group] = (max(r, ratio), n + 1)


# ---------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------
def bits(plane):
    """A plane's values (exact bf16 numbers) as bf16 bit patterns."""
    b = plane.to(torch.bfloat16)
    assert bool((b.double() == plane.double()).all()), "an operand plane holds a value that is no bf16 number"
    return b.view(torch.int16)


# helpers.guarded / read_guarded are exactly sized fp32 buffers; here a buffer has a pitch wider than its rows, rows a remap leaves out
# and, for the planes, 16-bit elements that have no NaN of torch's own to fill with: the same idea, kept local for those three reasons
def pitched32(dev, t, ldc, rows=None):
    """fp32 rows at pitch ldc in a NaN buffer with a guard row: (buffer, [rows, ldc] view)."""
    rows = t.shape[0] if rows is None else rows
    buf = torch.full((rows * ldc + 64,), float("nan"), device=dev)
    view = buf[:rows * ldc].view(rows, ldc)
    if t is not None and t.numel():
        view[:t.shape[0], :t.shape[1]] = t.float().to(dev)
    return buf, view


def pitched16(dev, t, ldc, rows=None):
    rows = t.shape[0] if rows is None else rows
    buf = torch.full((rows * ldc + 64,), NAN16, dtype=torch.int16, device=dev)
    view = buf[:rows * ldc].view(rows, ldc)
    if t is not None and t.numel():
        view[:t.shape[0], :t.shape[1]] = bits(t).to(dev)
    return buf, view


def read_rows(buf, view, rows, N, what):
    """The [M, N] block the kernel wrote, after asserting that nothing else was: pad columns, rows the remap does not name, guard row."""
    host, nrows, ldc = buf.cpu(), view.shape[0], view.shape[1]
    filled = torch.isnan(host) if host.dtype == torch.float32 else host == NAN16
    assert bool(filled[nrows * ldc:].all()), f"{what}: the guard row was written"
    body = filled[:nrows * ldc].view(nrows, ldc)
    assert bool(body[:, N:].all()), f"{what}: pad columns were written"
    named = torch.zeros(nrows, dtype=torch.bool)
    named[rows] = True
    assert bool(body[~named].all()), f"{what}: rows the remap does not name were written"
    assert not bool(body[rows][:, :N].any()), f"{what}: elements left unwritten"
    out = host[:nrows * ldc].view(nrows, ldc)[rows][:, :N]
    return out if out.dtype == torch.float32 else out.view(torch.bfloat16).double()


# ---------------------------------------------------------------------------------------------------
# one launch against the oracle
# ---------------------------------------------------------------------------------------------------
def ratio_of(got, want, floor32, extra=0.0, rounding=None):
    """helpers.check_against_floor as a number: error / bound with bound = MARGIN * fp32_floor.  Local because the bf16 allowances are
    per ELEMENT (half an ulp of each fp64 value, `extra`), which the scalar bound of check_against_floor cannot take, and because the
    largest ratio of every group is collected for the table.  With extra = 0 and rounding = None it is check_against_floor's ratio.
    rounding: the 'one fp32 rounding of the result' below which no bound goes (helpers.fp32_floor: EPS32 max|want|); a caller whose
    result is a SUM of rounded terms passes the rounding of its terms (statistics, below)."""
    floor = max(maxabs(floor32, want), EPS32 * float(want.abs().max()) if rounding is None else rounding)
    bound = torch.as_tensor(MARGIN * floor + extra, dtype=torch.float64).clamp_min(1e-300)      # (an all-zero ReLU output: 0 / tiny = 0)
    return float(((got.double() - want).abs() / bound).max())


def run_case(c, family, expect=None, alias=False, group=None, refs=None):
    """Launch case c on `family`, check every buffer, return {what: error / bound}.  refs: (fp64, fp32) references computed elsewhere."""
    import streamformer_amd._native as nat
    dev = gpu_device()
    M, N, K = c.shape
    ldc = N + PAD
    want, floor = refs if refs else (G.reference(c, torch.float64), G.reference(c, torch.float32))
    rows = want["rows"]
    nrows = int(rows.max()) + 1 + (3 if c.grp[0] > 0 else 0)
    keep = []

    def up16(p):
        t = bits(p).contiguous().to(dev)
        keep.append(t)
        return t.data_ptr()

    def up32(t):
        t = t.float().contiguous().to(dev)
        keep.append(t)
        return t.data_ptr()

    d = nat.SfGemmDesc()
    d.split = int(c.split)
    d.a_hi, d.w_hi = up16(c.a[0]), up16(c.w[0])
    if c.split:
        d.a_lo, d.w_lo = up16(c.a[1]), up16(c.w[1])
    if c.bias is not None:
        d.bias = up32(c.bias)
    d.M, d.N, d.K, d.epi, d.act, d.alpha, d.ldc = M, N, K, c.epi, c.act, c.alpha, ldc
    d.grp_rows, d.grp_stride, d.grp_off = c.grp
    d.ln_eps = c.ln_eps
    out32 = out16 = None
    planes_out = c.out_planes if (c.epi in (G.BF16, G.ACT_BF16) or c.resid_planes is not None) else 0
    if c.epi == G.RESID_F32:
        if c.resid_planes is not None:
            rb = [pitched16(dev, p, ldc, nrows) for p in c.resid_planes]
            d.resid_hi, d.resid_lo = rb[0][1].data_ptr(), rb[1][1].data_ptr()
            if len(rb) == 3:
                d.resid_lo2 = rb[2][1].data_ptr()
            if alias:
                out16 = rb[:planes_out]
            keep.append(rb)
        else:
            rb = pitched32(dev, c.resid, ldc, nrows if c.resid_mod == 0 else None)
            d.resid, d.resid_mod = rb[1].data_ptr(), c.resid_mod
            if c.resid_mod == 0 and c.grp[0] > 0:       # the residual is read at the REMAPPED row (the cache row it is added to)
                rb[1].fill_(float("nan"))
                rb[1][rows.to(dev), :N] = c.resid.float().to(dev)
            if alias:
                assert c.resid_mod == 0
                out32 = rb
            keep.append(rb)
    if c.epi == G.EMBED_F32:
        d.pos, d.time_rows, d.Np, d.Tn = up32(c.pos), up32(c.time_rows), c.pos.shape[0], c.time_rows.shape[0]
    if planes_out:
        if out16 is None:
            out16 = [pitched16(dev, torch.empty(0, 0), ldc, nrows) for _ in range(planes_out)]
        d.out_hi = out16[0][1].data_ptr()
        if planes_out > 1:
            d.out_lo = out16[1][1].data_ptr()
        if planes_out > 2:
            d.out_lo2 = out16[2][1].data_ptr()
    else:
        if out32 is None:
            out32 = pitched32(dev, torch.empty(0, 0), ldc, nrows)
        d.out_f32 = out32[1].data_ptr()
        if c.extra.get("also_hi"):       # a fold producer on an fp32 residual: the bf16 copy of the new rows next to them
            also_hi = pitched16(dev, torch.empty(0, 0), ldc, nrows)
            d.out_hi = also_hi[1].data_ptr()
    stats = None
    if c.stats_kind:
        pairs, width = G.stats_layout(c.stats_kind, N)
        stats = pitched32(dev, torch.zeros(M, width), width)       # cleared as run_forward clears it, once per forward ...
        for at, _, _ in pairs:
            stats[1][:, at:at + 2] = float("nan")                  # ... and NaN where the producer must write
        d.ln_stats_out, d.ln_stats_wide = stats[1].data_ptr(), 1
    if c.ln_s is not None:
        d.ln_s = up32(c.ln_s)
        if c.ln_inkernel:
            d.ln_inkernel = 1
        else:
            d.ln_stats, d.ln_stats_wide = up32(c.ln_stats), int(c.ln_stats.shape[1] == 8)
    taken = C.c_int(-1)
    nat.check(nat.lib.sf_op_gemm(C.byref(d), family, C.byref(taken), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert taken.value == (expect if expect is not None else family), f"ran on {FAMILY.get(taken.value, taken.value)}"
    res = {}
    v64, v32 = want["value"], floor["value"]
    if planes_out:
        got = [read_rows(b, v, rows, N, f"plane {i}") for i, (b, v) in enumerate(out16)]
        total = sum(got)
        for p in got:
            assert bool(torch.isfinite(p).all())
        assert bool(G.is_nearest_bf16(got[0], total).all()), "out_hi is not a nearest bf16 number to the planes' sum"
        if planes_out > 1:
            half = 0.5 * G.bf16_ulp(got[0])
            assert bool((got[1].abs() <= half).all()), "|lo| > half an ulp of hi"
            off_tie = (total - got[0]).abs() < half       # the other neighbour only where the planes' sum is an exact tie
            assert bool((got[0] == G.bf16_round(total))[off_tie].all()), "out_hi != bf16_round(hi + lo (+ lo2)) off a tie"
        extra = {1: 0.5 * G.bf16_ulp(v64), 2: G.TWO_PLANES_REL * v64.abs(), 3: G.THREE_PLANES_REL * v64.abs()}[planes_out]
        res["value"] = ratio_of(total, v64, v32, extra)
    else:
        got = read_rows(*out32, rows, N, "out_f32")
        assert bool(torch.isfinite(got).all())
        res["value"] = ratio_of(got, v64, v32)
        if c.extra.get("also_hi"):
            hi = read_rows(*also_hi, rows, N, "out_hi")
            assert bool((hi == G.bf16_round(got.double())).all()), "out_hi is not bf16 of the fp32 row written next to it"
    if stats is not None:
        host = stats[0].cpu()
        assert bool(torch.isnan(host[M * 8:]).all()), "statistics: the guard row was written"
        srows = host[:M * 8].view(M, 8)
        assert not bool(torch.isnan(srows).any()), "statistics: a pair the layout names was not written"
        written = {at + j for at, _, _ in pairs for j in (0, 1)}
        for j in set(range(8)) - written:
            assert bool((srows[:, j] == 0).all()), f"statistics: float {j} of the row is not in the layout and was written"
        for j, name in ((0, "sum x"), (1, "sum x^2")):
            cols = [at + j for at, _, _ in pairs]
            # sum x and sum x^2 are held to bounds of their own (one bound over the whole row would be set by sum x^2, 20 to 200 times
            # larger, and is what helpers.check_against_floor gives).  Each is a sum of n fp32 values that carry a rounding of their
            # own, so one rounding of the RESULT is EPS32 sum |term|, not EPS32 |sum|: for sum x^2 the two are the same number, for a
            # sum x that cancels they are not, and the fp32 floor model itself misses 4 EPS32 |sum x| on a share of all rows
            # (test_gemm_oracle_cpu.py, test_a_cancelling_sum_is_not_held_to_roundings_of_its_result).  Never more than the rounding
            # check_against_floor would use for the whole buffer.
            terms = v64 if j == 0 else v64 * v64
            per_pair = torch.stack([terms[:, c0:c1].abs().sum(dim=1) for _, c0, c1 in pairs], dim=1)
            rounding = EPS32 * min(float(per_pair.max()), float(want["stats"].abs().max()))
            res[name] = ratio_of(srows[:, cols], want["stats"][:, cols], floor["stats"][:, cols], rounding=rounding)
    mode = "bf16x3" if c.split else "bf16"
    for what, r in res.items():
        g = f"{FAMILY[taken.value]} | {mode} | {group or EPI[c.epi]}" + ("" if what == "value" else f" [{what}]")
        note(g, r)
        assert r <= 1.0, (g, what, r, (M, N, K))
    return res


# ---------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------
def rows_mixed(seed, M, K):
    """Rows of ordinary scale, and every second row with mean 8 and standard deviation 0.5: where a LayerNorm fold cancels."""
    x = randn(seed, M, K)
    x[1::2] = x[1::2] * 0.5 + 8.0
    return x


def make(seed, M, N, K, split, epi, x=None, W=None, bias=True, **kw):
    n = 2 if split else 1
    x = randn(seed, M, K) if x is None else x
    W = randn(seed + 1, N, K) / K ** 0.5 if W is None else W
    c = G.Case(a=[p.double() for p in G.split_planes(x.float(), n)], w=[p.double() for p in G.split_planes(W.float(), n)], epi=epi,
               bias=randn(seed + 2, N) if bias is True else bias, **kw)
    if epi in (G.BF16, G.ACT_BF16) and "out_planes" not in kw:
        c.out_planes = n
    return c


def variant(seed, M, N, K, split, name, family):
    """The epilogue variants every family is asked for, by name."""
    how = "bf16" if not split else ("fast" if family == G256 else "ocml")
    grp = (32, 40, 3)
    if name == "F32":
        return make(seed, M, N, K, split, G.F32)
    if name == "F32 remap":
        return make(seed, M, N, K, split, G.F32, grp=grp)
    if name == "BF16":
        return make(seed, M, N, K, split, G.BF16)
    if name == "BF16 remap":
        return make(seed, M, N, K, split, G.BF16, grp=grp)
    if name.startswith("ACT"):
        return make(seed, M, N, K, split, G.ACT_BF16, act=int(name[-1]), act_how=how, x=randn(seed, M, K) * 1.5)
    if name == "RESID":
        return make(seed, M, N, K, split, G.RESID_F32, resid=randn(seed + 3, M, N), alpha=0.75)
    if name == "RESID remap":
        return make(seed, M, N, K, split, G.RESID_F32, resid=randn(seed + 3, M, N), alpha=0.75, grp=grp)
    if name == "EMBED":      # Np * Tn = 21 divides none of the M used
        return make(seed, M, N, K, split, G.EMBED_F32, pos=randn(seed + 4, 7, N), time_rows=randn(seed + 5, 3, N))
    raise ValueError(name)


def fold_case(seed, M, N, K, split, epi, act=0, how="bf16", inkernel=True, stats_kind="tile256"):
    """A fold consumer ALONE: A = the planes of x, statistics = fp64 sums of x rounded to fp32 (in-kernel: the kernel sums the A rows it
    reads, and so do the references), W' / ln_s / b' from (W, gamma, beta, b)."""
    x = rows_mixed(seed, M, K)
    W, b = randn(seed + 1, N, K) / K ** 0.5, randn(seed + 2, N)
    gamma, beta = 1.0 + 0.2 * randn(seed + 6, K), 0.3 * randn(seed + 7, K)
    wp, ln_s, bp = G.fold_operands(W, gamma, beta, b, split)
    n = 2 if split else 1
    c = G.Case(a=[p.double() for p in G.split_planes(x, n)], w=wp, epi=epi, bias=bp, act=act, act_how=how, ln_s=ln_s, ln_inkernel=inkernel,
               out_planes=n if epi != G.F32 else 1)
    if not inkernel:
        c.ln_stats = G.stats_rows(x.double(), stats_kind).float()
    return c


# ---------------------------------------------------------------------------------------------------
# 128^2
# ---------------------------------------------------------------------------------------------------
G128_VARIANTS = ["F32", "F32 remap", "BF16", "BF16 remap", "ACT 0", "ACT 1", "ACT 2", "RESID", "EMBED"]


@pytest.mark.parametrize("name", G128_VARIANTS)
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_g128(split, name):
    seed = 100
    for K in ((32, 96) if split else (64, 192)):
        for M in (1, 127, 128, 129, 300):
            for N in (4, 124, 128, 132, 384):
                if K in (96, 192) and (M, N) not in ((1, 4), (129, 132), (300, 384), (127, 124)):
                    continue      # the second K: the corners and the ragged diagonal
                seed += 10
                run_case(variant(seed, M, N, K, split, name, G128), G128)


def test_g128_column_split_through_dispatch():
    """N = 256 j + 128: the 256-column kernel on 1024 columns and the 128^2 kernel on the last 128, one row past a 256-row tile.
    (2049, 1152, 128) splits in the accurate mode; in the bf16 mode the skinny family takes every M <= 2560 and the tile family
    2560 < M <= 6272 first, as documented, so the bf16 split is run one row past the tile family's range."""
    run_case(variant(900, 2049, 1152, 128, True, "F32", G256), AUTO, expect=COLSPLIT, group="F32 (column split)")
    run_case(variant(910, 2049, 1152, 128, True, "RESID", G256), AUTO, expect=COLSPLIT, group="RESID (column split)")
    run_case(variant(920, 2049, 1152, 128, False, "F32", G256), AUTO, expect=SKINNY, group="F32 (dispatch at 2049 x 1152)")
    run_case(variant(930, 6273, 1152, 128, False, "F32", G256), AUTO, expect=COLSPLIT, group="F32 (column split)")
    run_case(variant(940, 6273, 1152, 128, False, "BF16", G256), AUTO, expect=COLSPLIT, group="BF16 (column split)")


# ---------------------------------------------------------------------------------------------------
# skinny
# ---------------------------------------------------------------------------------------------------
SKINNY_SHAPES = [(1, 4, 64), (31, 36, 128), (32, 64, 448), (33, 100, 64), (196, 768, 128), (513, 768, 64), (513, 36, 448), (196, 4, 128),
                 (1, 768, 448), (33, 100, 512),      # tiles <= 256 and K >= 512: the K-parallel instance
                 (513, 768, 512),                    # 408 tiles: the 32 x 32 instance at a long K (bf16: the 64 x 64 tiles above 512 rows)
                 (3000, 32, 128)]                    # the rank-32 LoRA projection


@pytest.mark.parametrize("name", ["F32", "F32 remap", "BF16", "BF16 remap", "ACT 0", "ACT 1", "ACT 2", "RESID", "RESID remap", "EMBED"])
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_skinny(split, name):
    for i, (M, N, K) in enumerate(SKINNY_SHAPES):
        run_case(variant(2000 + 10 * i, M, N, K, split, name, SKINNY), SKINNY)
    if name == "RESID" and not split:       # the streamed K = 768 residual projection: K-parallel with three K-tiles per group, unrolled
        run_case(variant(2500, 196, 768, 768, False, name, SKINNY), SKINNY, group="RESID (K = 768 unrolled)")


@pytest.mark.parametrize("epi,act", [(G.BF16, 0), (G.ACT_BF16, 0), (G.ACT_BF16, 1)])
def test_skinny_fold_in_kernel(epi, act):
    # K / 64 = 2, 3, 4, 5: every tiles-per-slot instance; (33, 100, 512): K-parallel; (196, 3072, 256): the 32 x 96 wide tiles
    for i, (M, N, K) in enumerate([(196, 768, 128), (31, 36, 192), (33, 100, 256), (129, 64, 320), (33, 100, 512), (196, 3072, 256), (1, 4, 64)]):
        run_case(fold_case(3000 + 10 * i, M, N, K, False, epi, act), SKINNY, group=f"fold in kernel {EPI[epi]}")


@pytest.mark.parametrize("epi", [G.F32, G.BF16, G.ACT_BF16])
def test_skinny_fold_in_kernel_accurate(epi):
    """Accurate mode: the 32 x 32 instance only (more than 256 tiles), K / 64 a multiple of four and not."""
    for i, (M, N, K) in enumerate([(513, 768, 128), (513, 772, 256)]):
        run_case(fold_case(3200 + 10 * i, M, N, K, True, epi, 0, "ocml"), SKINNY, group=f"fold in kernel {EPI[epi]}")


def test_skinny_refuses_what_it_does_not_read():
    """resid_mod is read by the panel kernel alone: on any other family the call is refused by name, nothing is launched."""
    import streamformer_amd._native as nat
    c = make(3300, 33, 64, 64, False, G.RESID_F32, resid=randn(3301, 8, 64), resid_mod=8)
    with pytest.raises(nat.NativeError, match="resid_mod"):
        run_case(c, SKINNY)
    with pytest.raises(nat.NativeError, match="does not take"):
        run_case(make(3310, 4000, 768, 64, True, G.F32), SKINNY)       # accurate mode: M <= 1024 unless N <= 64


# ---------------------------------------------------------------------------------------------------
# tile
# ---------------------------------------------------------------------------------------------------
TILE_M = (1, 127, 129, 300, 2561)      # 300: ragged in the 128-row and the 256-row tiles


@pytest.mark.parametrize("shape_id", ["auto", 0, 1, 2, 3, 4, 5])
def test_tile(switches, shape_id):
    # sf_launch_gemm_tile takes a forced id only if that shape takes the call (shape_takes in csrc/sf_gemm_tile.hip: N a multiple of its
    # column tile; F32 / RESID / EMBED on ids 0 .. 2 only; the fold on ids 3 and 4 only) and falls back to its own choice otherwise, and
    # family_taken names the family, not the instance.  N and the epilogues below are chosen so that every id takes every one of its
    # cases; whoever edits kShapes / shape_takes or these lists keeps the two in step, or a case runs on another instance unseen.
    switches("SF_TILE_MIN_M", 0)
    if shape_id != "auto":
        switches("SF_TILE_SHAPE", shape_id)
    wide = shape_id in (3, 4, 5)
    N = {"auto": 768, 0: 192, 1: 288, 2: 384, 3: 512, 4: 768, 5: 512}[shape_id]
    names = ["BF16", "ACT 0", "ACT 1"] if wide else ["F32", "RESID", "EMBED", "BF16", "ACT 2"]
    seed = 4000
    for M in TILE_M:
        for K in (128, 192):
            if K == 192 and M not in (129, 2561):
                continue
            for name in names:
                seed += 10
                run_case(variant(seed, M, N, K, False, name, TILE), TILE, group=f"{name.split()[0]} (shape {shape_id})")
            if shape_id in ("auto", 3, 4):
                for epi in (G.BF16, G.ACT_BF16):
                    seed += 10
                    run_case(fold_case(seed, M, N, K, False, epi), TILE, group=f"fold in kernel {EPI[epi]} (shape {shape_id})")


@pytest.mark.parametrize("name", ["RESID", "EMBED"])
def test_tile_statistics_producer(switches, name):
    """The 128 x 192 statistics producers: hi plane + one pair per 192-column quarter, N / 192 = 2 and 4."""
    switches("SF_TILE_MIN_M", 0)
    switches("SF_TILE_FOLD_MIN_M", 0)
    for i, (M, N, K) in enumerate([(1, 384, 128), (129, 768, 192), (300, 768, 128), (2561, 384, 128)]):
        c = variant(4800 + 10 * i, M, N, K, False, name, TILE)
        c.stats_kind = "quarter"
        c.extra["also_hi"] = True
        d32 = run_case(c, TILE, group=f"{name} + statistics")
        assert "sum x" in d32


# ---------------------------------------------------------------------------------------------------
# panel
# ---------------------------------------------------------------------------------------------------
def panel_ms():
    """M on each side of the steps of the panel plan's m-tile count (2 / 4 / 7 / 13 tiles of 16 rows per panel; panels = a multiple of
    half the CUs covering ceil(M / 208)), for the device's CU count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count & ~15
    half = cus // 2
    return [100, 32 * half, 32 * half + 1, 64 * half + 1, 112 * half + 1]


def plane_resid_case(seed, M, N, K, split, nplanes, kind):
    c = make(seed, M, N, K, split, G.RESID_F32, alpha=1.0)
    r = rows_mixed(seed + 3, M, N)
    c.resid_planes = [p.double() for p in G.split_planes(r, nplanes)]
    c.out_planes, c.stats_kind = nplanes, kind
    return c


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("K", [128, 160])
def test_panel(switches, K, i):
    """At M = 100 most panels are empty.  The fill threshold is lowered so that every m-tile count is reached at both of its edges; every
    epilogue runs at every M, each M being another instance of the kernel."""
    switches("SF_PANEL_MIN_FILL_PCT", 1)
    for M in (panel_ms()[i],):
        seed = 5000 + 100 * i + K
        run_case(variant(seed, M, 768, K, False, "F32", PANEL), PANEL)
        for alias in (False, True):
            run_case(plane_resid_case(seed + 10, M, 768, K, False, 2, "panel"), PANEL, alias=alias, group="RESID planes + wide statistics")
        run_case(variant(seed + 20, M, 768, K, False, "BF16", PANEL), PANEL)
        for alias in (False, True):
            run_case(variant(seed + 30, M, 768, K, False, "RESID", PANEL), PANEL, alias=alias)
        c = make(seed + 40, M, 768, K, False, G.RESID_F32, resid=randn(seed + 43, 57, 768), resid_mod=57)
        run_case(c, PANEL, group="RESID resid_mod")


# ---------------------------------------------------------------------------------------------------
# 256^2
# ---------------------------------------------------------------------------------------------------
G256_M = (2048, 2049, 2303, 2305)


@pytest.mark.parametrize("name", ["F32", "BF16", "BF16 remap", "ACT 0", "RESID"])
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_g256(split, name):
    seed = 6000
    for M in G256_M:
        for K in (128, 256, 384):
            if K != 128 and M != 2305:
                continue
            seed += 10
            run_case(variant(seed, M, 1024, K, split, name, G256), G256)
    if name == "ACT 0" and split:
        run_case(variant(seed + 10, 2049, 1024, 128, True, "ACT 1", G256), G256)


@pytest.mark.parametrize("name", ["BF16", "ACT 0", "fold BF16", "fold ACT_BF16"])
def test_g256_bf16_mode_on_256_row_tiles(switches, name):
    """The bf16 mode does not read SF_G256_FORCE_BM: at N = 1024 every M of G256_M fits one round of the grid either way, 224-row tiles
    cost less, and every bf16-mode case above runs on them.  Without them (SF_G256_NO_BM224) the 256-row instance — the one the
    benchmark's shapes take — runs the bf16 outputs and the fold consumers."""
    switches("SF_G256_NO_BM224")
    for i, M in enumerate((2049, 2305)):
        if name.startswith("fold"):
            epi = G.BF16 if name == "fold BF16" else G.ACT_BF16
            c = fold_case(6900 + 10 * i, M, 1024, 256, False, epi, 0, "bf16", inkernel=False)
            run_case(c, G256, group=f"fold consumer {EPI[epi]} (row tiles no224)")
        else:
            run_case(variant(6950 + 10 * i, M, 1024, 128, False, name, G256), G256, group=f"{name.split()[0]} (row tiles no224)")


@pytest.mark.parametrize("bm", [160, 192, 224, 256, "no224"])
def test_g256_row_tile_heights(switches, bm):
    if bm == "no224":
        switches("SF_G256_NO_BM224")
    else:
        switches("SF_G256_FORCE_BM", bm)       # read by the accurate mode
    for i, M in enumerate((2049, 2305)):
        for split in ((False, True) if bm == "no224" else (True,)):
            run_case(variant(6500 + 10 * i, M, 1024, 128, split, "F32", G256), G256, group=f"F32 (row tiles {bm})")
            run_case(plane_resid_case(6600 + 10 * i, M, 1024, 128, split, 3 if split else 2, "tile256"), G256, alias=bool(i),
                     group=f"RESID planes + statistics (row tiles {bm})")


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_g256_plane_producers(split):
    """hi + lo (bf16 mode) and hi + lo + lo2 (accurate mode) in and out, one statistics pair per 256-column tile (N = 768 in the accurate
    mode: three pairs, the fourth stays zero)."""
    for i, (M, N, K) in enumerate([(2048, 1024, 128), (2303, 1024, 256), (2305, 1024, 384)] + ([(6400, 768, 128)] if split else [])):
        for alias in (False, True):
            run_case(plane_resid_case(6700 + 10 * i, M, N, K, split, 3 if split else 2, "tile256"), G256, alias=alias,
                     group="RESID planes + statistics")


@pytest.mark.parametrize("epi,act", [(G.BF16, 0), (G.ACT_BF16, 0)])
@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_g256_fold_consumers_alone(split, epi, act):
    for i, (M, N, K) in enumerate([(2049, 1024, 256), (2305, 1280, 256), (2048, 1024, 768), (2303, 1280, 1024)]):
        kind = "tile256" if K % 256 == 0 and K <= 1024 else "quarter"
        run_case(fold_case(6800 + 10 * i, M, N, K, split, epi, act, "fast" if split else "bf16", inkernel=False, stats_kind=kind), G256,
                 group=f"fold consumer {EPI[epi]}")


# ---------------------------------------------------------------------------------------------------
# producer -> consumer
# ---------------------------------------------------------------------------------------------------
def chain(name, prod_family, cons_family, split, M, D, N2, K1, form, stats_kind=None, epi=G.BF16, act=0, how="bf16", seed=7000):
    """A residual producer and the fold consumer behind it, both on the device, the consumer reading the planes (and statistics) the
    producer KERNEL wrote.  form "planes": plane residual in and out (three planes in the accurate mode) with statistics; "fp32": fp32
    residual, fp32 rows out with their bf16 copy (accurate mode: hi + lo) and, with stats_kind, the statistics; stats_kind None: the
    consumer sums its rows itself (ln_inkernel).

    Reference: the producer's result x in fp64, then oracle_ops.layernorm(x, gamma, beta) and operand_linear with exact operands (then the
    activation) — no fold formula, no rounding.  Floor model: the chain as the kernels run it, in fp32 — x, its planes, statistics of x
    (or of the planes, in-kernel), W' = W gamma rounded, the fold epilogue, the kernel's activation — so it carries the operand
    rounding and the fold's cancellation, and nothing else is allowed for them.  (Buffers here have their exact sizes: pitch, pads and
    guards of every producer and consumer are run_case's business.)"""
    import streamformer_amd._native as nat
    dev = gpu_device()
    n = 2 if split else 1
    if form == "planes":
        p = plane_resid_case(seed, M, D, K1, split, 3 if split else 2, stats_kind)
    else:
        p = make(seed, M, D, K1, split, G.RESID_F32, resid=rows_mixed(seed + 3, M, D), alpha=1.0)
    W, b = randn(seed + 11, N2, D) / D ** 0.5, randn(seed + 12, N2)
    gamma, beta = 1.0 + 0.2 * randn(seed + 16, D), 0.3 * randn(seed + 17, D)
    eps = 1e-6
    x64 = G.reference(p, torch.float64)["value"]
    want = G.operand_linear(G.layernorm(x64, gamma.double(), beta.double(), eps), W.double(), b.double())
    if epi == G.ACT_BF16:
        want = G.kernel_activation(want, act, "exact")
    x32 = G.reference(p, torch.float32)["value"]
    wp, ln_s, bp = G.fold_operands(W, gamma, beta, b, split)
    c = G.Case(a=[q.double() for q in G.split_planes(x32, n)], w=wp, epi=epi, bias=bp, act=act, act_how=how, ln_s=ln_s, ln_eps=eps,
               ln_inkernel=stats_kind is None, out_planes=n)
    if stats_kind is not None:
        c.ln_stats = G.stats_rows(x32, stats_kind)
    floor = G.reference(c, torch.float32)["value"]

    st = torch.cuda.current_stream(dev).cuda_stream
    keep = []

    def up16(t):
        keep.append(bits(t).contiguous().to(dev))
        return keep[-1].data_ptr()

    def up32(t):
        keep.append(t.float().contiguous().to(dev))
        return keep[-1].data_ptr()

    def new16(rows, cols):
        keep.append(torch.full((rows, cols), NAN16, dtype=torch.int16, device=dev))
        return keep[-1]

    d = nat.SfGemmDesc()
    d.split = int(split)
    d.a_hi, d.w_hi = up16(p.a[0]), up16(p.w[0])
    if split:
        d.a_lo, d.w_lo = up16(p.a[1]), up16(p.w[1])
    d.bias = up32(p.bias)
    d.M, d.N, d.K, d.epi, d.alpha, d.ldc = M, D, K1, G.RESID_F32, p.alpha, D
    if form == "planes":
        planes = [bits(q).contiguous().to(dev) for q in p.resid_planes]
        d.resid_hi = d.out_hi = planes[0].data_ptr()
        d.resid_lo = d.out_lo = planes[1].data_ptr()
        if len(planes) == 3:
            d.resid_lo2 = d.out_lo2 = planes[2].data_ptr()
    else:
        rows32 = p.resid.float().contiguous().to(dev)
        planes = [new16(M, D) for _ in range(n)]
        d.resid = d.out_f32 = rows32.data_ptr()
        d.out_hi = planes[0].data_ptr()
        if split:
            d.out_lo = planes[1].data_ptr()
    stats = torch.zeros(M, 8, device=dev)
    if stats_kind is not None:
        d.ln_stats_out, d.ln_stats_wide = stats.data_ptr(), 1
    taken = C.c_int(-1)
    nat.check(nat.lib.sf_op_gemm(C.byref(d), prod_family, C.byref(taken), st))
    assert taken.value == prod_family
    e = nat.SfGemmDesc()
    e.split = int(split)
    e.a_hi, e.w_hi = planes[0].data_ptr(), up16(c.w[0])
    if split:
        e.a_lo, e.w_lo = planes[1].data_ptr(), up16(c.w[1])
    e.bias, e.ln_s, e.ln_eps = up32(c.bias), up32(c.ln_s), eps
    if stats_kind is not None:
        e.ln_stats, e.ln_stats_wide = stats.data_ptr(), 1
    else:
        e.ln_inkernel = 1
    e.M, e.N, e.K, e.epi, e.act, e.ldc = M, N2, D, epi, act, N2
    out = [new16(M, N2) for _ in range(n)]
    e.out_hi = out[0].data_ptr()
    if split:
        e.out_lo = out[1].data_ptr()
    nat.check(nat.lib.sf_op_gemm(C.byref(e), cons_family, C.byref(taken), st))
    torch.cuda.synchronize(dev)
    assert taken.value == cons_family
    host = [o.cpu() for o in out]
    assert not any(bool((h == NAN16).any()) for h in host), "output elements left unwritten"
    got = sum(h.view(torch.bfloat16).double() for h in host)
    extra = {1: 0.5 * G.bf16_ulp(want), 2: G.TWO_PLANES_REL * want.abs()}[n]
    r = ratio_of(got, want, floor, extra)
    note(f"chain {name} | {'bf16x3' if split else 'bf16'} | {EPI[epi]}", r)
    assert r <= 1.0, (name, r)


def test_chain_panel_to_g256(switches):
    switches("SF_PANEL_MIN_FILL_PCT", 1)
    chain("panel -> 256^2", PANEL, G256, False, 4097, 768, 1024, 128, "planes", "panel")
    chain("panel -> 256^2", PANEL, G256, False, 4097, 768, 1024, 128, "planes", "panel", epi=G.ACT_BF16, seed=7100)


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_chain_g256_to_g256(split):
    how = "fast" if split else "bf16"
    chain("256^2 -> 256^2", G256, G256, split, 2305, 1024, 1024, 128, "planes", "tile256", how=how, seed=7200)
    chain("256^2 -> 256^2", G256, G256, split, 2049, 1024, 1280, 128, "planes", "tile256", epi=G.ACT_BF16, how=how, seed=7300)


def test_chain_tile_statistics_producer_to_g256(switches):
    """The forward's path from SF_TILE_FOLD_MIN_M rows up: the 128 x 192 tile producer's quarter statistics, the 256^2 consumer."""
    switches("SF_TILE_MIN_M", 0)
    switches("SF_TILE_FOLD_MIN_M", 0)
    chain("tile (statistics) -> 256^2", TILE, G256, False, 2561, 768, 1024, 128, "fp32", "quarter", seed=7400)
    chain("tile (statistics) -> 256^2", TILE, G256, False, 2561, 768, 1024, 128, "fp32", "quarter", epi=G.ACT_BF16, seed=7500)


def test_chain_tile_to_tile_in_kernel(switches):
    """The forward's path below SF_TILE_FOLD_MIN_M rows: the tile producer's bf16 copy, the wide tile consumers summing it themselves."""
    switches("SF_TILE_MIN_M", 0)
    chain("tile -> tile (in kernel)", TILE, TILE, False, 300, 384, 768, 128, "fp32", seed=7600)
    chain("tile -> tile (in kernel)", TILE, TILE, False, 2561, 384, 512, 128, "fp32", epi=G.ACT_BF16, act=1, seed=7700)


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "bf16x3"])
def test_chain_skinny_to_skinny_in_kernel(split):
    """The streamed frame's path.  Accurate mode: hi + lo copies, and the 32 x 32 consumer instance (more than 256 tiles)."""
    M, how = (513, "ocml") if split else (196, "bf16")
    chain("skinny -> skinny (in kernel)", SKINNY, SKINNY, split, M, 128, 768, 64, "fp32", how=how, seed=7800)
    chain("skinny -> skinny (in kernel)", SKINNY, SKINNY, split, M, 256, 768, 128, "fp32", epi=G.ACT_BF16, how=how, seed=7900)


# ---------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------
def documented_family(M, N, K, epi, split):
    """The forward's choice from the thresholds README.md / DESIGN.md document (plain Linear calls: no fold, no planes):
      skinny   M <= 2560 (accurate mode: 1024) or N <= 64; K a multiple of 64
      tile     bf16 mode, 2560 < M <= 6272, K >= 128 a multiple of 64, N a multiple of a tile width its epilogue takes
               (F32 / RESID / EMBED: 96-wide tiles; BF16 / ACT: 96 or 256-wide)
      panel    bf16 mode, N = 768, F32 / BF16 / RESID, K >= 128 a multiple of 32, last-round fill >= 75 % (55 % from M = 14 000)
      256^2    M >= 2048, N a multiple of 256 and >= 1024 (accurate mode above 6272 rows: 768), K a multiple of 128, no EMBED,
               bf16 mode: erf GELU only
      column split   N = 256 j + 128 > 256 whose first 256 j columns the 256^2 kernel takes
      128^2    everything else"""
    if ((M <= (1024 if split else 2560)) or N <= 64) and K % 64 == 0 and N % 4 == 0:
        return SKINNY
    if not split and 2560 < M <= 6272 and K >= 128 and K % 64 == 0 and N % 8 == 0:
        narrow_only = epi in (G.F32, G.RESID_F32, G.EMBED_F32)
        if N % 96 == 0 or (not narrow_only and N % 256 == 0):
            return TILE
    if not split and N == 768 and epi in (G.F32, G.BF16, G.RESID_F32) and K >= 128 and K % 32 == 0:
        cus = torch.cuda.get_device_properties(0).multi_processor_count & ~15
        half = cus // 2
        panels = -(-(-(-M // 208)) // half) * half
        rows = -(-M // panels)
        mt = next((t for t in (2, 4, 7, 13) if rows <= 16 * t), 0)
        if mt and rows * 100 >= mt * 16 * (55 if M >= 14000 else 75):
            return PANEL

    def g256(n):
        return M >= 2048 and n % 256 == 0 and n >= (768 if split and M > 6272 else 1024) and K % 128 == 0 and epi != G.EMBED_F32
    if g256(N):
        return G256
    if N % 256 == 128 and N > 256 and epi != G.EMBED_F32 and g256(N - 128):
        return COLSPLIT
    return G128


def test_dispatch_takes_the_documented_family():
    """family 0 over the shapes of test_op_linear_shape_sweep and the forward's Linear calls of SigLIP-base at 1, 2, 5 and 8 clips:
    family_taken against the documented thresholds.  (The results are compared with the oracle in the per-family tests.)"""
    import numpy as np
    import streamformer_amd._native as nat
    dev = gpu_device()
    rng = np.random.default_rng(7)
    shapes = [(25088, 768, 768), (25088, 2304, 768), (6272, 768, 3072), (3136, 3072, 768), (784, 2304, 768), (1568, 768, 3072),
              (600, 1000, 128), (2048, 3072, 768), (4096, 1152, 1152), (2304, 3456, 1152), (3000, 1152, 4352)]
    for _ in range(14):
        shapes.append((int(rng.integers(513, 9000)), int(rng.choice([768, 1024, 1536, 2304, 3072])), int(rng.choice([128, 256, 384, 768, 1152]))))
    calls = [(M, N, K, epi) for M, N, K in shapes for epi in (G.F32, G.RESID_F32, G.ACT_BF16)]
    for clips in (1, 2, 5, 8):
        M = clips * 16 * 196
        calls += [(M, 768, 768, G.EMBED_F32), (M, 2304, 768, G.F32), (M, 2304, 768, G.BF16), (M, 768, 768, G.RESID_F32),
                  (M, 3072, 768, G.ACT_BF16), (M, 768, 3072, G.RESID_F32)]
    big = max(M * max(N, K) for M, N, K, _ in calls) + max(N * K for _, N, K, _ in calls)
    pool16 = torch.zeros(big, dtype=torch.int16, device=dev)
    big_out = max(M * N for M, N, _, _ in calls)
    out32, res32, out16 = torch.empty(big_out, device=dev), torch.zeros(big_out, device=dev), torch.empty(big_out, dtype=torch.int16, device=dev)
    small = torch.zeros(1 << 20, device=dev)
    wrong = []
    for split in (False, True):
        for M, N, K, epi in calls:
            d = nat.SfGemmDesc()
            d.split = int(split)
            d.a_hi = d.a_lo = d.w_hi = d.w_lo = pool16.data_ptr()
            if not split:
                d.a_lo = d.w_lo = None
            d.M, d.N, d.K, d.epi, d.alpha, d.ldc = M, N, K, epi, 1.0, N
            if epi in (G.BF16, G.ACT_BF16):
                d.out_hi = out16.data_ptr()
                if split:
                    d.out_lo = out16.data_ptr()
            else:
                d.out_f32 = out32.data_ptr()
            if epi == G.RESID_F32:
                d.resid = res32.data_ptr()
            if epi == G.EMBED_F32:
                d.pos, d.time_rows, d.Np, d.Tn = small.data_ptr(), small.data_ptr(), 196, 16
            taken = C.c_int(-1)
            nat.check(nat.lib.sf_op_gemm(C.byref(d), AUTO, C.byref(taken), torch.cuda.current_stream(dev).cuda_stream))
            want = documented_family(M, N, K, epi, split)
            if taken.value != want:
                wrong.append(((M, N, K), EPI[epi], "bf16x3" if split else "bf16", FAMILY[taken.value], FAMILY[want]))
    torch.cuda.synchronize(dev)
    assert not wrong, wrong


def test_refusals_name_the_field():
    import streamformer_amd._native as nat
    dev = gpu_device()
    buf = torch.zeros(1 << 16, dtype=torch.int16, device=dev)
    f = torch.zeros(1 << 16, device=dev)

    def base():
        d = nat.SfGemmDesc()
        d.a_hi = d.w_hi = buf.data_ptr()
        d.M, d.N, d.K, d.ldc, d.out_f32 = 64, 64, 64, 64, f.data_ptr()
        return d
    for edit, word in ((lambda d: setattr(d, "ldc", 60), "ldc"), (lambda d: setattr(d, "out_f32", None), "out_f32"),
                       (lambda d: setattr(d, "resid_mod", -1), "resid_mod"), (lambda d: setattr(d, "resid_hi", buf.data_ptr()), "resid_lo"),
                       (lambda d: setattr(d, "ln_s", f.data_ptr()), "ln_stats"), (lambda d: setattr(d, "a_lo", buf.data_ptr()), "split"),
                       (lambda d: setattr(d, "epi", 4), "pos"), (lambda d: setattr(d, "epi", 3), "resid"),
                       (lambda d: setattr(d, "out_lo", buf.data_ptr()), "out_hi")):
        d = base()
        edit(d)
        assert nat.lib.sf_op_gemm(C.byref(d), AUTO, None, None) == nat.SF_ERR_INVALID
        assert word.encode() in nat.lib.sf_last_error(), (word, nat.lib.sf_last_error())
    d = base()
    assert nat.lib.sf_op_gemm(C.byref(d), PANEL, None, None) == nat.SF_ERR_INVALID and b"panel" in nat.lib.sf_last_error()
