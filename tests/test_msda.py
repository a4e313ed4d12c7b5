"""Multi-scale deformable attention on the MI355X: the three entry points against fp64 (tests/msda_oracle.py) over a geometry sweep, border
and collision cases, the fused entry, the module in both compute modes against fixture F21, reproducibility, streams and graph capture.

Tolerances follow tests/test_oad.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds — the error, against fp64, of the
reference's operator sequence in torch (split per level, grid_sample, weighted sum; its autograd for the gradients) on the same inputs, in
plain fp32 for the operator and with bf16_operands="x3" / True on every Linear for the module's two modes — and never less than one fp32
rounding of the result.  The floor is computed here, on the CPU, from the inputs; never from the code under test.

In every gradient case the generator asserts, in fp64, that each sample's pixel coordinates are at least 1e-3 from an integer: the
location gradient jumps there.  That is a condition on the inputs, not a tolerance.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import msda_oracle as MO
from tests.conftest import ROOT
from tests.helpers import EPS32, MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded

pytestmark = pytest.mark.gpu

MODES = {"fp32": "x3", "bf16": True}
N = MO.N_BATCH

#        D   M  shapes                                  P  Lq
SWEEP = [(8, 1, [(6, 5), (3, 3), (1, 2)], 4, 7),
         (24, 3, [(3, 4)], 1, 1),
         (32, 8, [(6, 5), (3, 3), (1, 2)], 4, 37),
         (64, 3, [(5, 4), (3, 3), (2, 2), (1, 2)], 4, 7),
         (128, 3, [(6, 5), (3, 3), (1, 2)], 1, 37),
         (64, 8, [(3, 4)], 4, 1),
         (64, 3, [(2, 2)], 4, 147),                          # extractor-like: Lq >> S
         (32, 3, [(12, 12), (6, 6), (3, 3)], 4, 4)]          # injector-like: S >> Lq


def _levels(shapes):
    flat = [v for hw in shapes for v in hw]
    return (C.c_int32 * len(flat))(*flat), (C.c_int32 * len(shapes))(*MO.level_starts(shapes))


def _op_forward(value, shapes, loc, w):
    import streamformer_amd._native as nat
    dev = gpu_device()
    _, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    hw, st = _levels(shapes)
    v, l, a = (t.to(dev).contiguous() for t in (value, loc, w))
    buf, out = guarded(dev, N, Lq, M * D)
    nat.check(nat.lib.sf_op_msda_forward(v.data_ptr(), hw, st, l.data_ptr(), a.data_ptr(), out.data_ptr(), N, S, M, D, Lq, L, P,
                                         nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return read_guarded(buf, out)


def _op_backward(value, shapes, loc, w, grad_out):
    import streamformer_amd._native as nat
    dev = gpu_device()
    _, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    hw, st = _levels(shapes)
    v, l, a, g = (t.to(dev).contiguous() for t in (value, loc, w, grad_out))
    bufs, views = zip(*(guarded(dev, *t.shape) for t in (value, loc, w)))
    nat.check(nat.lib.sf_op_msda_backward(v.data_ptr(), hw, st, l.data_ptr(), a.data_ptr(), g.data_ptr(), views[0].data_ptr(), views[1].data_ptr(),
                                          views[2].data_ptr(), N, S, M, D, Lq, L, P, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return [read_guarded(buf, view) for buf, view in zip(bufs, views)]


def _draw(seed, D, M, shapes, P, Lq):
    rs = np.random.RandomState(seed)
    L = len(shapes)
    value = torch.from_numpy(rs.standard_normal((N, MO.pixels(shapes), M, D)).astype(np.float32))
    loc = MO.draw_locations(rs, N, Lq, M, shapes, P)
    w = torch.softmax(torch.from_numpy(rs.standard_normal((N, Lq, M, L * P)).astype(np.float32)), -1).view(N, Lq, M, L, P)
    grad_out = torch.from_numpy(rs.standard_normal((N, Lq, M * D)).astype(np.float32))
    return value, loc, w, grad_out


def _both_floors(value, shapes, loc, w, grad_out):
    """fp64 results of the explicit gather, and the fp32 results of the reference's torch sequence: (want, floor), each (out, gv, gl, gw)."""
    want = MO.core_with_grads(MO.core, value.double(), shapes, loc.double(), w.double(), grad_out.double())
    floor = MO.core_with_grads(MO.core_grid_sample, value, shapes, loc, w, grad_out)
    return want, floor


# ------------------------------------------------------------------------------------------------
# 1. the unfused entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,shapes,P,Lq", SWEEP)
def test_forward_and_backward_vs_fp64(D, M, shapes, P, Lq):
    value, loc, w, grad_out = _draw(2200 + D + M + Lq, D, M, shapes, P, Lq)
    want, floor = _both_floors(value, shapes, loc, w, grad_out)
    got = [_op_forward(value, shapes, loc, w)] + _op_backward(value, shapes, loc, w, grad_out)
    for name, g, f, t in zip(("out", "grad_value", "grad_sampling_locations", "grad_attention_weights"), got, floor, want):
        check_against_floor(name, g, f, t)
    # reproducibility: forward and the two owned gradients bit for bit; grad_value (float atomics) only to its floor, checked above
    again = [_op_forward(value, shapes, loc, w)] + _op_backward(value, shapes, loc, w, grad_out)
    for i in (0, 2, 3):
        assert torch.equal(got[i], again[i]), i
    check_against_floor("grad_value, second run", again[1], floor[1], want[1])


def test_f21_operator_cases():
    g = MO.load_golden()
    for name, c in MO.CORE_CASES.items():
        value, loc, w, grad_out = (torch.from_numpy(g[f"{name}.{k}"]) for k in ("value", "loc", "w", "grad_out"))
        _, floor = _both_floors(value, c["shapes"], loc, w, grad_out)
        got = [_op_forward(value, c["shapes"], loc, w)] + _op_backward(value, c["shapes"], loc, w, grad_out)
        for key, gg, f in zip(("out", "grad_value", "grad_loc", "grad_w"), got, floor):
            check_against_floor(f"{name}.{key}", gg, f, torch.from_numpy(g[f"{name}.{key}"]))


def test_samples_on_pixel_centres_and_limits():
    """Forward only: every pixel coordinate is an integer from -1 to H (W), exactly: centres, and the two excluded limits."""
    shapes, M, D, P = [(4, 4), (2, 2), (1, 2)], 3, 16, 4
    L = len(shapes)
    rs = np.random.RandomState(2301)
    Lq = 19
    loc = torch.empty(N, Lq, M, L, P, 2)
    for l, (H, W) in enumerate(shapes):
        kx = rs.randint(-1, W + 1, (N, Lq, M, P))
        ky = rs.randint(-1, H + 1, (N, Lq, M, P))
        loc[:, :, :, l, :, 0] = torch.from_numpy((kx + 0.5) / W)
        loc[:, :, :, l, :, 1] = torch.from_numpy((ky + 0.5) / H)
    px = MO.pixel_coordinates(loc, shapes)
    assert bool((px == px.round()).all()) and float(px.min()) == -1.0 and float(px[..., 0].max()) == 4.0
    assert bool(((loc * torch.tensor([[W, H] for H, W in shapes])[None, None, None, :, None, :] - 0.5) == px.float()).all()), "fp32 agrees exactly"
    value = torch.from_numpy(rs.standard_normal((N, MO.pixels(shapes), M, D)).astype(np.float32))
    w = torch.softmax(torch.from_numpy(rs.standard_normal((N, Lq, M, L * P)).astype(np.float32)), -1).view(N, Lq, M, L, P)
    want = MO.core(value.double(), shapes, loc.double(), w.double())
    check_against_floor("out", _op_forward(value, shapes, loc, w), MO.core_grid_sample(value, shapes, loc, w), want)


def test_scatter_collisions():
    """Every query of every head samples the same point: all adds of grad_value land on the same four pixels."""
    shapes, M, D, P, Lq = [(5, 4)], 3, 32, 4, 37
    value, _, w, grad_out = _draw(2302, D, M, shapes, P, Lq)
    loc = torch.empty(N, Lq, M, 1, P, 2)
    loc[..., 0], loc[..., 1] = 0.41, 0.63
    assert MO.away_from_integers(loc, shapes)
    want, floor = _both_floors(value, shapes, loc, w, grad_out)
    got = _op_backward(value, shapes, loc, w, grad_out)
    assert int((want[1].abs().sum((2, 3)) > 0).sum()) == 4 * N
    for name, g, f, t in zip(("grad_value", "grad_sampling_locations", "grad_attention_weights"), got, floor[1:], want[1:]):
        check_against_floor(name, g, f, t)


# ------------------------------------------------------------------------------------------------
# 2. the fused entry
# ------------------------------------------------------------------------------------------------
def _op_fused(value, mask, shapes, offsets, logits, ref):
    import streamformer_amd._native as nat
    dev = gpu_device()
    _, S, M, D = value.shape
    Lq, L = ref.shape[1], len(shapes)
    P = logits.shape[-1] // (M * L)
    hw, st = _levels(shapes)
    v, o, lg, r = (t.to(dev).contiguous() for t in (value, offsets, logits, ref))
    pad = None if mask is None else mask.to(dev, torch.uint8).contiguous()
    buf, out = guarded(dev, N, Lq, M * D)
    nat.check(nat.lib.sf_op_msda_forward_fused(v.data_ptr(), nat.ptr(pad), hw, st, o.data_ptr(), o.shape[-1], lg.data_ptr(), lg.shape[-1], r.data_ptr(),
                                               r.shape[-1], out.data_ptr(), N, S, M, D, Lq, L, P, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return read_guarded(buf, out)


@pytest.mark.parametrize("big_logits", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_entry(ref_dim, masked, big_logits):
    D, M, shapes, P, Lq = 32, 3, [(6, 5), (3, 3), (1, 2)], 4, 7
    L, S = len(shapes), MO.pixels(shapes)
    rs = np.random.RandomState(2400 + ref_dim + 10 * masked + 100 * big_logits)
    value = torch.from_numpy(rs.standard_normal((N, S, M, D)).astype(np.float32))
    offsets = torch.from_numpy((2.5 * rs.standard_normal((N, Lq, M * L * P * 2))).astype(np.float32))
    logits = torch.from_numpy(rs.standard_normal((N, Lq, M * L * P)).astype(np.float32))
    if big_logits:
        logits = logits + torch.from_numpy(rs.choice([-80.0, 0.0, 80.0], size=tuple(logits.shape)).astype(np.float32))
    ref = rs.uniform(-0.05, 1.05, (N, Lq, L, 2))
    if ref_dim == 4:
        ref = np.concatenate([ref, rs.uniform(0.1, 1.5, (N, Lq, L, 2))], -1)
    ref = torch.from_numpy(ref.astype(np.float32))
    mask = None
    if masked:
        mask = torch.from_numpy(rs.uniform(size=(N, S)) < 0.3)
        mask[1, MO.level_starts(shapes)[1]:MO.level_starts(shapes)[2]] = True      # the middle level of sample 1 wholly masked
    sides = {}
    for dt in (torch.float64, torch.float32):
        off = offsets.to(dt).view(N, Lq, M, L, P, 2)
        w = torch.softmax(logits.to(dt).view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        loc = MO.locations(off, ref.to(dt), shapes, P)
        v = value.to(dt) if mask is None else value.to(dt).masked_fill(mask[:, :, None, None], 0.0)
        sides[dt] = (v, loc, w)
    want = MO.core(*sides[torch.float64][:1], shapes, *sides[torch.float64][1:])
    v32, loc32, w32 = sides[torch.float32]
    floor = MO.core_grid_sample(v32, shapes, loc32, w32)
    got = _op_fused(value, mask, shapes, offsets, logits, ref)
    check_against_floor("fused vs fp64", got, floor, want)
    unfused = _op_forward(v32, shapes, loc32, w32)           # the unfused entry fed torch's masked value, locations and softmax
    bound = MARGIN * fp32_floor(floor, want)
    assert maxabs(got, unfused) <= bound, (maxabs(got, unfused), bound)
    assert torch.equal(_op_fused(value, mask, shapes, offsets, logits, ref), got)


# ------------------------------------------------------------------------------------------------
# 3. the module
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module_case(name):
    """(inputs, weights, fp64 output, {mode: floor output}) of a fixture case, computed once and shared."""
    g = MO.load_golden()
    c = MO.MODULE_CASES[name]
    query, flat, ref, go = (torch.from_numpy(g[f"{name}.{k}"]).float() for k in ("query", "input_flatten", "reference_points", "grad_out"))
    mask = torch.from_numpy(g[f"{name}.mask"]) if f"{name}.mask" in g else None
    sd = MO.make_weights(c)
    want = MO.module(sd, c, query, flat, ref, mask)
    floors = {m: MO.module(sd, c, query, flat, ref, mask, dtype=torch.float32, bf16_operands=bo, sample=MO.core_grid_sample) for m, bo in MODES.items()}
    return (query, flat, ref, mask, go), sd, want, floors, torch.from_numpy(g[f"{name}.out"])


def _module(name, mode):
    import streamformer_amd as sa
    c = MO.MODULE_CASES[name]
    m = sa.MSDeformAttn(c["d_model"], len(c["shapes"]), c["heads"], c["P"], ratio=0.5, compute_dtype=mode)
    m.load_state_dict(MO.make_weights(c))
    return m.to(gpu_device())


def _run(m, c, query, ref, flat, mask, shapes_as=list):
    dev = gpu_device()
    shapes, starts = c["shapes"], MO.level_starts(c["shapes"])
    if shapes_as is not list:
        shapes, starts = shapes_as(shapes), shapes_as(starts)
    return m(query.to(dev), ref.to(dev), flat.to(dev), shapes, starts, None if mask is None else mask.to(dev))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["tiny", "pix", "ada1", "ada3"])
def test_module_vs_f21_and_oracle(name, mode):
    (query, flat, ref, mask, _), sd, want, floors, stored = _module_case(name)
    c = MO.MODULE_CASES[name]
    m = _module(name, mode).eval()
    with torch.no_grad():
        got = _run(m, c, query, ref, flat, mask).cpu()
        on_device = _run(m, c, query, ref, flat, mask, shapes_as=lambda v: torch.tensor(v, device=gpu_device())).cpu()
    check_against_floor(f"{name} {mode} vs oracle", got, floors[mode], want)
    check_against_floor(f"{name} {mode} vs F21", got, floors[mode], stored)
    assert torch.equal(on_device, got), "shapes given as device tensors change the result"
    # the grad path (plain torch projections + the autograd function) agrees within the mode's floor
    for p in m.parameters():
        p.requires_grad_(True)
    with_grad = _run(m, c, query, ref, flat, mask).detach().cpu()
    bound = MARGIN * fp32_floor(floors[mode], want)
    assert maxabs(with_grad, got) <= bound, (maxabs(with_grad, got), bound)
    check_against_floor(f"{name} grad path vs oracle", with_grad, floors["fp32"], want)


@pytest.mark.parametrize("name", ["tiny", "tiny4"])
def test_module_parameter_gradients_vs_f21(name):
    g = MO.load_golden()
    (query, flat, ref, mask, go), sd, want, _, _ = _module_case(name)
    c = MO.MODULE_CASES[name]
    _, floor = MO.module_with_grads(sd, c, query, flat, ref, mask, go, dtype=torch.float32, sample=MO.core_grid_sample)
    m = _module(name, "fp32")
    dev = gpu_device()
    q, f = query.to(dev).requires_grad_(True), flat.to(dev).requires_grad_(True)
    out = m(q, ref.to(dev), f, torch.tensor(c["shapes"]), torch.tensor(MO.level_starts(c["shapes"])), None if mask is None else mask.to(dev))
    out.backward(go.to(dev))
    got = {k: p.grad.cpu() for k, p in m.named_parameters()}
    got.update(query=q.grad.cpu(), input_flatten=f.grad.cpu())
    assert set(got) == set(floor)
    for k in got:
        check_against_floor(f"{name} d/d {k}", got[k], floor[k], torch.from_numpy(g[f"{name}.grad.{k}"]))


# ------------------------------------------------------------------------------------------------
# 4. streams, graphs, the tool, the stand-in
# ------------------------------------------------------------------------------------------------
def test_non_default_stream_is_honoured():
    import streamformer_amd as sa
    dev = gpu_device()
    D, M, shapes, P, Lq = 32, 3, [(6, 5), (3, 3), (1, 2)], 4, 37
    value, loc, w, _ = _draw(2501, D, M, shapes, P, Lq)
    v, l, a = value.to(dev), loc.to(dev), w.to(dev)
    want = sa.ms_deform_attn(v, shapes, None, l, a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    staged = torch.zeros_like(v)
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):                      # keeps the side stream busy: a kernel on another stream would read `staged` too early
            big = (big @ big).clamp_(-1, 1)
        staged.copy_(v)
        got = sa.ms_deform_attn(staged, shapes, None, l, a)
    side.synchronize()
    assert torch.equal(got, want)
    torch.cuda.synchronize()


def test_graph_capture_of_the_fused_forward():
    name, mode = "pix", "fp32"
    (query, flat, ref, mask, _), _, _, _, _ = _module_case(name)
    c = MO.MODULE_CASES[name]
    dev = gpu_device()
    m = _module(name, mode).eval()
    shapes = torch.tensor(c["shapes"], device=dev)
    starts = torch.tensor(MO.level_starts(c["shapes"]), device=dev)
    q, r, f, k = query.to(dev), ref.to(dev), flat.to(dev), mask.to(dev)
    with torch.no_grad():
        eager = m(q, r, f, shapes, starts, k).clone()          # reads the shapes back once; sizes the workspace
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(q, r, f, shapes, starts, k)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(q, r, f, shapes, starts, k)                # a second read-back would synchronise and break the capture
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        q.copy_(q.flip(1))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m(q, r, f, shapes, starts, k))


def test_compiled_op_stand_in_runs():
    import streamformer_amd as sa
    dev = gpu_device()
    c = MO.CORE_CASES["c0"]
    value, loc, w, grad_out = (t.to(dev) for t in MO.make_core_inputs(c))
    op = sa.as_compiled_op()
    shapes, starts = torch.tensor(c["shapes"], device=dev), torch.tensor(MO.level_starts(c["shapes"]), device=dev)
    out = op.ms_deform_attn_forward(value, shapes, starts, loc, w, 64)
    gv, gl, gw = op.ms_deform_attn_backward(value, shapes, starts, loc, w, grad_out, 64)
    v, l, a = (t.clone().requires_grad_(True) for t in (value, loc, w))
    y = sa.MSDeformAttnFunction.apply(v, shapes, starts, l, a, 64)
    y.backward(grad_out)
    assert torch.equal(y.detach(), out) and torch.equal(l.grad, gl) and torch.equal(a.grad, gw)
    # grad_value is a sum of float atomics in arrival order: a pixel of this case takes at most Lq * P = 20 adds per head, and two orders
    # of k adds differ by at most k - 1 roundings of partial sums that stay below the sum of the magnitudes
    assert maxabs(v.grad, gv) <= 20 * EPS32 * max(1.0, float(gv.abs().max()))


def test_bench_tool_smoke():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "msda_bench.py"), "--smoke"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
