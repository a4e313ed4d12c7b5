"""The ViT-Adapter on the MI355X: its two kernels against fp64 torch over the grids and widths at which they take another path, and the
whole module in both compute modes against fixture F22 (the reference's own class in fp64; tests/vit_adapter_oracle.py).

Tolerances follow tests/test_msda.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds — the error, against fp64, of
the same operator sequence in torch on the same inputs at the operand precision of the mode under test (plain fp32 for the two kernels;
bf16_operands="x3" / True on every GEMM for the module's two modes) — and never less than one fp32 rounding of the result.  The floor is
computed here, on the CPU, from the inputs; never from the code under test.

Measured on an MI355X (largest error / bound over all cases): depthwise kernel 0.40, fusion kernel 0.27, module 0.35 in fp32 mode and 0.32 in
bf16 mode.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vit_adapter_oracle as VO
from tests.conftest import ROOT
from tests.helpers import check_against_floor, gpu_device, guarded, read_guarded
from tests.oracle_ops import operand_linear

pytestmark = pytest.mark.gpu

MODES = {"fp32": "x3", "bf16": True}
GRIDS = [(2, 2), (4, 6), (14, 14)]
FRAMES = 2


# ------------------------------------------------------------------------------------------------
# 1. depthwise 3 x 3 + GELU on the three-level token tensor
# ------------------------------------------------------------------------------------------------
def _op_dwconv(x, w, b, H, W):
    import streamformer_amd._native as nat
    dev = gpu_device()
    Fr, _, C = x.shape
    xd, wd, bd = x.to(dev).contiguous(), w.reshape(C, 3, 3).to(dev).contiguous(), b.to(dev).contiguous()
    buf, y = guarded(dev, *x.shape)
    nat.check(nat.lib.sf_op_adapter_dwconv_gelu(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), Fr, H, W, C, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return read_guarded(buf, y)


def _dwconv_sides(x, w, b, H, W):
    want = F.gelu(VO.dwconv(x.double(), w.double(), b.double(), H, W))
    return want, F.gelu(VO.dwconv(x, w, b, H, W))


@pytest.mark.parametrize("C", [32, 48, 192])
@pytest.mark.parametrize("H,W", GRIDS)
def test_dwconv_gelu_vs_fp64(H, W, C):
    rs = np.random.RandomState(2600 + 100 * H + W + C)
    n = (H // 2) * (W // 2)
    x = torch.from_numpy(rs.standard_normal((FRAMES, 21 * n, C)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((C, 1, 3, 3)) / 3.0).astype(np.float32))
    b = torch.from_numpy((0.1 * rs.standard_normal(C)).astype(np.float32))
    want, floor = _dwconv_sides(x, w, b, H, W)
    got = _op_dwconv(x, w, b, H, W)
    check_against_floor(f"dwconv {H}x{W} C={C}", got, floor, want)
    assert torch.equal(_op_dwconv(x, w, b, H, W), got), "two runs differ"
    # every level of every frame holds its own large constant: a tap that crosses a level or a frame boundary shows at once
    flat = torch.empty(FRAMES, 21 * n, C)
    for f in range(FRAMES):
        for l, (a, e) in enumerate(((0, 16 * n), (16 * n, 20 * n), (20 * n, 21 * n))):
            flat[f, a:e] = 1000.0 * (1 + 3 * f + l) * (-1.0) ** l
    want, floor = _dwconv_sides(flat, w, b, H, W)
    check_against_floor(f"dwconv {H}x{W} C={C}, constant levels", _op_dwconv(flat, w, b, H, W), floor, want)


# ------------------------------------------------------------------------------------------------
# 2. the tail's fusion kernel
# ------------------------------------------------------------------------------------------------
SCALE = {0: 4, 1: 2, 2: 1, 3: 0.5}


def _linear_gpu(x, w, mode="fp32"):
    import streamformer_amd._native as nat
    dev = gpu_device()
    M, K = x.shape
    N = w.shape[0]
    xd, wd = x.to(dev).contiguous(), w.to(dev).contiguous()
    y = torch.empty(M, N, device=dev)
    ws = torch.empty(max(nat.lib.sf_op_linear_workspace_bytes(M, N, K), 256), dtype=torch.uint8, device=dev)
    nat.check(nat.lib.sf_op_linear(xd.data_ptr(), wd.data_ptr(), None, None, 1.0, 0, y.data_ptr(), M, N, K, nat.compute_mode(mode), ws.data_ptr(),
                                   ws.numel(), nat.current_stream_handle(dev)))
    return y


def _fuse_case(level, H, W, D, seed):
    """Inputs of one level on a ViT grid of H x W, and both sides of the reference sequence: (inputs, want fp64, floor fp32) per vit flag."""
    rs = np.random.RandomState(seed)
    scale = SCALE[level]
    Ho, Wo = int(H * scale), int(W * scale)
    draw = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))      # noqa: E731
    vit = draw(FRAMES, H * W, D)
    bn = dict(weight=1.0 + 0.1 * draw(D), bias=0.1 * draw(D), mean=0.1 * draw(D), var=torch.from_numpy(rs.uniform(0.5, 1.5, D).astype(np.float32)))
    inp = dict(vit=vit, bn=bn)
    if level == 0:
        inp["c2"] = draw(FRAMES, 4 * H * W, D)                          # the stride-8 tokens the transposed convolution reads
        inp["up_w"], inp["up_b"] = draw(D, D, 2, 2) / D ** 0.5, 0.1 * draw(D)
        inp["c1"] = draw(FRAMES, D, Ho, Wo)
    else:
        inp["buf"] = draw(FRAMES, Ho * Wo + 5, D)                       # the level sits inside longer frames, as a slice of [F, 21 n, D] does
    sides = {}
    for dt in (torch.float64, torch.float32):
        if level == 0:
            if dt == torch.float64:
                m = F.conv_transpose2d(VO.tokens_to_map(inp["c2"].to(dt), 2 * H, 2 * W), inp["up_w"].to(dt), inp["up_b"].to(dt), 2)
            else:
                wl = inp["up_w"].permute(2, 3, 1, 0).reshape(4 * D, D)
                m = operand_linear(inp["c2"], wl, inp["up_b"].repeat(4), "x3").reshape(FRAMES, 2 * H, 2 * W, 2, 2, D)
                m = m.permute(0, 5, 1, 3, 2, 4).reshape(FRAMES, D, Ho, Wo)
            m = m + inp["c1"].to(dt)
        else:
            m = VO.tokens_to_map(inp["buf"][:, 3:3 + Ho * Wo].to(dt), Ho, Wo)
        vm = VO.tokens_to_map(vit.to(dt), H, W)
        vm = vm if level == 2 else F.interpolate(vm, scale_factor=scale, mode="bilinear", align_corners=False)
        norm = lambda t: F.batch_norm(t, bn["mean"].to(dt), bn["var"].to(dt), bn["weight"].to(dt), bn["bias"].to(dt), False, 0.0, VO.BN_EPS)      # noqa: E731
        sides[dt] = {True: norm(m + vm), False: norm(m)}
    return inp, sides[torch.float64], sides[torch.float32]


def _op_fuse(level, H, W, D, inp, with_vit):
    import streamformer_amd._native as nat
    dev = gpu_device()
    scale = SCALE[level]
    Ho, Wo = int(H * scale), int(W * scale)
    bn = inp["bn"]
    s64 = bn["weight"].double() / torch.sqrt(bn["var"].double() + VO.BN_EPS)
    t64 = bn["bias"].double() - bn["mean"].double() * s64
    c1 = None
    if level == 0:
        t64 = t64 + s64 * inp["up_b"].double()
        wl = inp["up_w"].permute(2, 3, 1, 0).reshape(4 * D, D)
        if D % 32 == 0:
            tok = _linear_gpu(inp["c2"].reshape(-1, D), wl)      # a real GEMM output [F * 2H * 2W, 4 D]
        else:                                                    # a width the GEMM does not take: the same product at its operand precision
            tok = operand_linear(inp["c2"].reshape(-1, D), wl, None, "x3").to(dev).contiguous()
        tok_ptr, stride = tok.data_ptr(), 4 * H * W * 4 * D
        c1 = inp["c1"].to(dev).contiguous()
    else:
        tok = inp["buf"].to(dev).contiguous()
        tok_ptr, stride = tok.data_ptr() + 4 * 3 * D, (Ho * Wo + 5) * D
    vit = inp["vit"].to(dev).contiguous() if with_vit else None
    sc, sh = s64.float().to(dev), t64.float().to(dev)
    buf, out = guarded(dev, FRAMES, D, Ho, Wo)
    nat.check(nat.lib.sf_op_adapter_fuse(level, tok_ptr, stride, nat.ptr(vit), nat.ptr(c1), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), FRAMES, H, W, D,
                                         nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return read_guarded(buf, out)


# D 8 and 72: less than one tile of channels, and one tile and a part; (10, 26): 65 pixels at res5, one tile and one pixel
@pytest.mark.parametrize("D", [8, 64, 72, 96])
@pytest.mark.parametrize("H,W", GRIDS + [(10, 26)])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_fuse_vs_fp64(level, H, W, D):
    inp, want, floor = _fuse_case(level, H, W, D, 2700 + 1000 * level + 10 * H + W + D)
    for with_vit in (True, False):
        got = _op_fuse(level, H, W, D, inp, with_vit)
        check_against_floor(f"res{level + 2} {H}x{W} D={D} vit={with_vit}", got, floor[with_vit], want[with_vit])
        assert torch.equal(_op_fuse(level, H, W, D, inp, with_vit), got), "two runs differ"


# ------------------------------------------------------------------------------------------------
# 3. the whole module against F22
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return VO.load_golden()


@functools.lru_cache(maxsize=None)
def _floors(name, mode):
    """The fp32 restatement at the mode's operand precision: (outputs, final c), computed once per case and mode."""
    c = VO.CASES[name]
    res, cs = VO.forward(VO.make_weights(c), c, VO.make_pixels(c), dtype=torch.float32, operands=MODES[mode])
    return res, cs[-1]


def _model(name, mode, sd=None):
    import streamformer_amd as sa
    c = VO.CASES[name]
    m = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(VO.config(c), compute_dtype=mode, **VO.adapter_kwargs(c))
    m.load_state_dict(VO.make_weights(c) if sd is None else sd, strict=True)
    return m.to(gpu_device()).eval()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(VO.CASES))
def test_module_vs_f22(name, mode):
    g, c = _golden(), VO.CASES[name]
    m = _model(name, mode)
    pixels = VO.make_pixels(c).to(gpu_device())
    outs, tokens = m.forward_with_tokens(pixels)
    assert list(outs) == list(VO.OUTPUTS)
    assert all(v.dtype == torch.float32 and not v.requires_grad and v.is_contiguous() for v in outs.values())
    floor_out, floor_c = _floors(name, mode)
    last = len(c["indexes"]) - 1
    check_against_floor(f"{name} {mode} c", tokens.cpu(), floor_c, torch.from_numpy(g[f"{name}.c{last}"]))
    for k in VO.OUTPUTS:
        want = torch.from_numpy(g[f"{name}.{k}"])
        assert tuple(outs[k].shape) == tuple(want.shape)
        check_against_floor(f"{name} {mode} {k}", outs[k].cpu(), floor_out[k], want)
    again = m(pixels)
    assert all(torch.equal(again[k], outs[k]) for k in VO.OUTPUTS), "two forwards differ"


def test_checkpoint_dtype_does_not_change_the_result():
    """bf16-representable weights loaded from an fp64 and from a bf16 state dict: the same fp32 parameters, bitwise equal outputs."""
    name = "sq"
    c = VO.CASES[name]
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in VO.make_weights(c).items()}
    pixels = VO.make_pixels(c).to(gpu_device())
    base = _model(name, "fp32", sd)(pixels)
    for dt in (torch.float64, torch.bfloat16):
        got = _model(name, "fp32", {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()})(pixels)
        assert all(torch.equal(got[k], base[k]) for k in VO.OUTPUTS), dt


# ------------------------------------------------------------------------------------------------
# 4. streams, the tool
# ------------------------------------------------------------------------------------------------
def test_non_default_stream_is_honoured():
    import streamformer_amd._native as nat
    dev = gpu_device()
    H, W, C = 4, 6, 64
    n = (H // 2) * (W // 2)
    rs = np.random.RandomState(2801)
    x = torch.from_numpy(rs.standard_normal((FRAMES, 21 * n, C)).astype(np.float32)).to(dev)
    w = torch.from_numpy(rs.standard_normal((C, 3, 3)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rs.standard_normal(C).astype(np.float32)).to(dev)
    ones = torch.ones(C, device=dev)

    def run(src):
        y, out = torch.empty_like(src), torch.empty(FRAMES, C, H, W, device=dev)
        s = nat.current_stream_handle(dev)
        nat.check(nat.lib.sf_op_adapter_dwconv_gelu(src.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), FRAMES, H, W, C, s))
        nat.check(nat.lib.sf_op_adapter_fuse(2, y.data_ptr() + 4 * 16 * n * C, 21 * n * C, src.data_ptr() + 4 * 16 * n * C, None, ones.data_ptr(), b.data_ptr(),
                                             out.data_ptr(), 1, H, W, C, s))
        return y, out

    want = run(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    staged = torch.zeros_like(x)
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):                      # keeps the side stream busy: a kernel on another stream would read `staged` too early
            big = (big @ big).clamp_(-1, 1)
        staged.copy_(x)
        got = run(staged)
    side.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1][:1], want[1][:1])
    torch.cuda.synchronize()


def test_bench_tool_smoke():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vit_adapter_bench.py"), "--smoke"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
