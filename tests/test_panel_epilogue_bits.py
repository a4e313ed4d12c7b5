"""GPU: the panel kernel's plane-residual epilogue alone (hi + lo bf16 residual planes read, both written back, {sum x, sum x^2} per
row half), through sf_op_gemm as tests/test_gemm_families.py drives it, against the operand-matched fp64 oracle of tests/gemm_oracle.py
at that file's floors; and the determinism of a launch, byte for byte.

Shapes: N = 768; K = 128 and 768 (the kernel takes no K below 128: 128 is four K-tiles, one lap of its four-slot ring with neither
steady-state loop entered, 768 runs the loop); one M per m-tile count of the plan (2 / 4 / 7 / 13 tiles of 16 rows, each another instance
of the kernel).  With P = half the CU count panels: M = 32 P has full panels of 32 rows; 32 P + 1, 64 P + 1 and 112 P + 1 give 33, 65 and
113 rows per panel (none a multiple of the 64-row staging group, the last m-tile partly rows that do not exist) and a ragged or empty
last panel.  alpha = 0.75 as well as 1: with alpha != 1 the product alpha * acc is rounded before it meets the residual, which is where
the epilogue's planes and statistics could part (csrc/sf_gemm_panel.hip, plane_row8)."""
import ctypes as C

import pytest
import torch

from tests import gemm_oracle as G
from tests import test_gemm_families as T
from tests.helpers import gpu_device, randn

pytestmark = pytest.mark.gpu


def plan_ms():
    half = (torch.cuda.get_device_properties(0).multi_processor_count & ~15) // 2
    return {2: 32 * half, 4: 32 * half + 1, 7: 64 * half + 1, 13: 112 * half + 1}


def plane_case(seed, M, K, alpha):
    c = T.plane_resid_case(seed, M, 768, K, False, 2, "panel")
    c.alpha = alpha
    return c


@pytest.mark.parametrize("mt", [2, 4, 7, 13])
@pytest.mark.parametrize("K", [128, 768])
def test_plane_epilogue_against_fp64(switches, K, mt):
    switches("SF_PANEL_MIN_FILL_PCT", 1)
    M = plan_ms()[mt]
    c = plane_case(9000 + 10 * mt + K, M, K, 0.75)
    refs = (G.reference(c, torch.float64), G.reference(c, torch.float32))
    for alias in (False, True):          # planes written in place, as the forward does, and to buffers of their own
        res = T.run_case(c, T.PANEL, alias=alias, group="RESID planes + wide statistics (alpha 0.75)", refs=refs)
        print(f"K {K} MT {mt} M {M} alias {alias}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
        assert {"value", "sum x", "sum x^2"} <= set(res)


def test_plane_epilogue_mostly_empty_panels(switches):
    """M = 100: one row per panel at most, every other row of every tile clamped or zero."""
    switches("SF_PANEL_MIN_FILL_PCT", 1)
    for alpha in (1.0, 0.75):
        T.run_case(plane_case(9300, 100, 128, alpha), T.PANEL, group="RESID planes + wide statistics (M 100)")


def launch_bytes(c, dev):
    """One launch of case c on the panel family: the bytes of the hi plane, the lo plane and the statistics rows."""
    import streamformer_amd._native as nat
    M, N, K = c.shape
    ldc = N + T.PAD
    keep = [T.bits(p).contiguous().to(dev) for p in (c.a[0], c.w[0])] + [c.bias.float().contiguous().to(dev)]
    resid = [T.pitched16(dev, p, ldc, M) for p in c.resid_planes]
    out = [T.pitched16(dev, torch.empty(0, 0), ldc, M) for _ in range(2)]
    stats = T.pitched32(dev, torch.zeros(M, 8), 8)
    d = nat.SfGemmDesc()
    d.a_hi, d.w_hi, d.bias = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    d.M, d.N, d.K, d.epi, d.alpha, d.ldc = M, N, K, c.epi, c.alpha, ldc
    d.resid_hi, d.resid_lo = resid[0][1].data_ptr(), resid[1][1].data_ptr()
    d.out_hi, d.out_lo = out[0][1].data_ptr(), out[1][1].data_ptr()
    d.ln_stats_out, d.ln_stats_wide = stats[1].data_ptr(), 1
    taken = C.c_int(-1)
    nat.check(nat.lib.sf_op_gemm(C.byref(d), T.PANEL, C.byref(taken), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert taken.value == T.PANEL
    return [b[0].cpu() for b in out] + [stats[0].cpu().view(torch.int32)]


@pytest.mark.parametrize("mt", [4, 13])
def test_two_launches_give_identical_bytes(switches, mt):
    switches("SF_PANEL_MIN_FILL_PCT", 1)
    dev = gpu_device()
    c = plane_case(9500 + mt, plan_ms()[mt], 128, 0.75)
    first, second = launch_bytes(c, dev), launch_bytes(c, dev)
    for name, a, b in zip(("hi plane", "lo plane", "statistics"), first, second):
        assert torch.equal(a, b), f"{name}: two launches of one shape differ"
    M = c.shape[0]
    st = first[2][:M * 8].view(torch.float32).view(M, 8)
    assert bool(torch.isfinite(st[:, [0, 1, 4, 5]]).all()) and bool((st[:, [2, 3, 6, 7]] == 0).all())
