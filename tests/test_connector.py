"""The native video-LLM connector on the MI355X: its pool-and-layout kernel against torch on the CPU, the whole connector against the
reference's stored outputs (tests/golden/f19_connector.npz) and the fp64 restatement in the reference's order
(tests/connector_oracle.py), one full-width case, frame-by-frame calls, the streaming window and the refusals.

Tolerances follow tests/test_text_tower.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds — the error, against
fp64, of the same operator sequence in torch in the REFERENCE's order at the operand precision of the mode (bf16_operands="x3" for the
accurate mode, True for the bf16 mode; plain fp32 for the kernel alone) — and never less than one fp32 rounding of the result.  The floor
is computed here, on the CPU, from the inputs; never from the code under test.  The native connector pools in FRONT of the last Linear
(average and bilinear commute with it); the floor is taken in the reference's order all the same.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as Fn

from tests import connector_oracle as CO
from tests.helpers import MARGIN, bf16_bits, fp32_floor, frames, from_bf16_bits, gpu_device, maxabs, randn, small_cfg

pytestmark = pytest.mark.gpu

BF16_ROUND = 2.0 ** -8          # one bf16 rounding of a result, relative (round-to-nearest-even loses at most 2^-9)
# hi = bf16(y), lo = bf16(y - hi): |y - hi| <= 2^-9 |y| and |(y - hi) - lo| <= 2^-9 |y - hi|, so hi + lo holds y to 2^-18 |y|; 2^-17 leaves
# room for y's own distance from the fp64 value the bound is written against
PLANES_ROUND = 2.0 ** -17
MODES = {"none": 0, "average": 1, "max": 2, "bilinear": 3}
NEWLINES = {"no_token": 0, "one_token": 1, "frame": 2, "grid": 3}


# ------------------------------------------------------------------------------------------------
# 1. sf_op_connector_pool
# ------------------------------------------------------------------------------------------------
def _torch_pool(x, P, mode, stride):
    """x [F, P * P, C] -> [F, P'^2, C] by torch's own operators on the CPU, in x's dtype."""
    F, _, Cc = x.shape
    g = x.reshape(F, P, P, Cc).permute(0, 3, 1, 2)
    if mode == "average":
        g = Fn.avg_pool2d(g, stride)
    elif mode == "max":
        g = Fn.max_pool2d(g, stride)
    elif mode == "bilinear":
        g = Fn.interpolate(g, size=[-(-P // stride)] * 2, mode="bilinear")
    return g.permute(0, 2, 3, 1).reshape(F, -1, Cc)


def _pool_call(nat, dev, *, x=None, hi=None, lo=None, F, P, Cc, mode, stride, nl, newline, out_dtype=None, out_lo=True):
    """One launch into NaN-filled buffers with one guard row past the end; returns the CPU copies (guard row included)."""
    Po = CO.pooled_side(P, mode, stride)
    pos = [k for k, v in NEWLINES.items() if v == nl][0]
    rows = CO.add_newline(torch.zeros(F, Po * Po, 1), torch.zeros(1), pos).shape[0]          # the oracle's row rule, not a copy of the library's
    nd = None if newline is None else newline.to(dev).contiguous()
    s = nat.current_stream_handle(dev)
    if x is not None:
        xd = x.to(dev).contiguous()
        out = torch.full((rows + 1, Cc), float("nan"), dtype=out_dtype, device=dev)
        code = nat.SF_F32 if out_dtype == torch.float32 else nat.SF_BF16
        nat.check(nat.lib.sf_op_connector_pool(xd.data_ptr(), None, None, F, P, Cc, MODES[mode], stride, nl, nat.ptr(nd), out.data_ptr(), code,
                                               None, None, s))
        torch.cuda.synchronize()
        return rows, (out.cpu(),)
    hd = hi.to(dev).contiguous()
    ld = None if lo is None else lo.to(dev).contiguous()
    nan_bits = torch.full((rows + 1, Cc), float("nan"), dtype=torch.bfloat16, device=dev).view(torch.int16)
    oh = nan_bits.clone()
    ol = nan_bits.clone() if out_lo else None
    nat.check(nat.lib.sf_op_connector_pool(None, hd.data_ptr(), nat.ptr(ld), F, P, Cc, MODES[mode], stride, nl, nat.ptr(nd), None, 0, oh.data_ptr(),
                                           nat.ptr(ol), s))
    torch.cuda.synchronize()
    return rows, (oh.cpu(),) + ((ol.cpu(),) if out_lo else ())


POOL_CASES = [(5, 2, "bilinear"), (5, 2, "average"), (5, 2, "max"), (6, 2, "bilinear"), (9, 4, "bilinear"), (3, 4, "bilinear"), (2, 2, "average"),
              (14, 2, "bilinear"), (7, 1, "none")]


@pytest.mark.parametrize("P,stride,mode", POOL_CASES)
def test_pool_kernel_vs_torch(P, stride, mode):
    import streamformer_amd._native as nat
    dev = gpu_device()
    worst = 0.0
    for Cc, F in ((64, 1), (64, 3), (200, 1), (200, 3)):
        x = randn(1900 + 17 * P + Cc + F, F, P * P, Cc) * 1.5
        newline = randn(7, Cc)
        # plane form: the tensor the planes hold (hi + lo, or hi alone) is the input of that form's reference
        hi, lo = bf16_bits(x), bf16_bits(x - x.to(torch.bfloat16).float())
        x_planes = {True: (from_bf16_bits(hi) + from_bf16_bits(lo)), False: from_bf16_bits(hi)}
        refs = {}
        for tag, xin in (("f32", x.double()), ("hilo", x_planes[True]), ("hi", x_planes[False])):
            want = _torch_pool(xin, P, mode, stride)
            f32 = _torch_pool(xin.float(), P, mode, stride)
            refs[tag] = (want, f32, fp32_floor(f32, want))
        for pos, nl in NEWLINES.items():
            is_nl = CO.add_newline(torch.zeros(F, refs["f32"][0].shape[1], 1), torch.ones(1), pos)[:, 0] == 1
            assert int(is_nl.sum()) == {"no_token": 0, "one_token": 1, "frame": F, "grid": F * CO.pooled_side(P, mode, stride)}[pos]
            runs = []
            for out_dtype in (torch.float32, torch.bfloat16):
                runs.append(("f32", out_dtype, dict(x=x, out_dtype=out_dtype)))
            runs.append(("hilo", "planes", dict(hi=hi, lo=lo, out_lo=True)))
            runs.append(("hi", "plane", dict(hi=hi, lo=None, out_lo=False)))
            for tag, form, kw in runs:
                want, f32, floor = refs[tag]
                seq = CO.add_newline(want, newline.double(), pos)
                seq32 = CO.add_newline(f32, newline, pos)
                rows, bufs = _pool_call(nat, dev, F=F, P=P, Cc=Cc, mode=mode, stride=stride, nl=nl, newline=newline if nl else None, **kw)
                assert rows == seq.shape[0]
                if form in ("planes", "plane"):
                    body = [b[:rows] for b in bufs]
                    for b in bufs:
                        assert torch.isnan(b[rows:].view(torch.bfloat16).float()).all(), "the guard row was written"
                        assert not torch.isnan(b[:rows].view(torch.bfloat16).float()).any(), "output elements left unwritten"
                    got = sum(from_bf16_bits(b) for b in body)
                    rel = PLANES_ROUND if form == "planes" else BF16_ROUND
                    exact_hi = bf16_bits(seq32)
                    if mode in ("max", "none"):                      # no arithmetic: the split of torch's own fp32 result, bit for bit
                        assert torch.equal(body[0], exact_hi)
                        if form == "planes":
                            assert torch.equal(body[1], bf16_bits(seq32 - seq32.to(torch.bfloat16).float()))
                    assert torch.equal(body[0][is_nl], exact_hi[is_nl])
                else:
                    out = bufs[0]
                    assert torch.isnan(out[rows:]).all(), "the guard row was written"
                    assert not torch.isnan(out[:rows]).any(), "output elements left unwritten"
                    got = out[:rows].double()
                    rel = 0.0 if form == torch.float32 else BF16_ROUND
                    exact = seq32 if form == torch.float32 else seq32.to(torch.bfloat16)
                    if mode in ("max", "none"):
                        assert torch.equal(out[:rows], exact), "max / copy must equal torch on the CPU exactly"
                    assert torch.equal(out[:rows][is_nl], exact[is_nl]), "newline rows must be the parameter itself"
                excess = ((got - seq).abs() - rel * seq.abs()).max().item()
                worst = max(worst, (got - seq).abs().max().item() / floor if rel == 0.0 else 0.0)
                assert excess <= MARGIN * floor, (Cc, F, pos, tag, form, excess, floor)
                again = _pool_call(nat, dev, F=F, P=P, Cc=Cc, mode=mode, stride=stride, nl=nl, newline=newline if nl else None, **kw)[1]
                assert all(torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a[:rows], b.view(torch.int16) if b.dtype == torch.bfloat16 else b[:rows])
                           for a, b in zip(again, bufs)), "two runs differ"
    print(f"[connector pool P={P} stride={stride} {mode}] largest fp32 error / floor {worst:.2f}")


def test_max_pool_propagates_nan_as_torch_does():
    import streamformer_amd._native as nat
    dev = gpu_device()
    x = randn(1990, 2, 25, 64)
    x[0, 6, 3] = float("nan")               # patch (1, 1): the last tap of cell (0, 0)'s window ...
    x[1, 0, 9] = float("nan")               # ... and patch (0, 0), the first tap of the same cell in the next frame
    want = _torch_pool(x, 5, "max", 2)
    assert int(torch.isnan(want).sum()) == 2
    rows, (out,) = _pool_call(nat, dev, x=x, F=2, P=5, Cc=64, mode="max", stride=2, nl=0, newline=None, out_dtype=torch.float32)
    assert torch.equal(torch.isnan(out[:rows]), torch.isnan(want.reshape(rows, 64)))
    assert torch.equal(torch.nan_to_num(out[:rows]), torch.nan_to_num(want.reshape(rows, 64)))


# ------------------------------------------------------------------------------------------------
# 2. the whole connector on every F19 configuration
# ------------------------------------------------------------------------------------------------
_GOLD = {}
_REFS = {}
FLOOR_OPERANDS = {"fp32": "x3", "bf16": True}


def _gold():
    if not _GOLD:
        _GOLD.update(CO.load_golden())
    return _GOLD


def _reference(sd, cfg, feats, key):
    """fp64 restatement in the reference's order and the two modes' floors: computed once per key, shared, never changed."""
    if key not in _REFS:
        want = CO.forward(sd, cfg, feats)
        _REFS[key] = dict(want=want, floor={m: fp32_floor(CO.forward(sd, cfg, feats, dtype=torch.float32, bf16_operands=op), want)
                                            for m, op in FLOOR_OPERANDS.items()})
    return _REFS[key]


def _connector(cfg, sd, mode, out_dtype=torch.float32):
    import streamformer_amd as sa
    m = sa.VideoTokenConnector(cfg, compute_dtype=mode, out_dtype=out_dtype)
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})
    return m.to(gpu_device())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CO.CASES))
def test_connector_vs_fixture_and_fp64(name, mode):
    dev = gpu_device()
    sd, cfg, feats, stored = CO.golden_case(_gold(), name)
    ref = _reference(sd, cfg, feats, name)
    m = _connector(cfg, sd, mode)
    out = m(feats.to(dev))
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.shape == ref["want"].shape == (m.num_tokens(CO.FRAMES, CO.CASES[name][2]), CO.D_OUT) and got.dtype == torch.float32
    err, floor = maxabs(got, ref["want"]), ref["floor"][mode]
    own = maxabs(stored, ref["want"])
    ref_err = maxabs(got, stored)
    print(f"[connector {name} {mode}] vs fp64 {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}  vs reference fp32 {ref_err:.3e}")
    # measured on an MI355X: see DESIGN.md 3.9 (largest ratio over all cases next to MARGIN there)
    assert err <= MARGIN * floor, (err, floor)
    assert ref_err <= MARGIN * floor + own, ref_err           # the fixture sits `own` away from fp64 itself
    if mode == "fp32":
        assert err <= 1e-3
    assert torch.equal(m(feats.to(dev)), out), "two runs differ"
    if name == "mlp_bil_p5_grid":
        # bf16 output: the same rows rounded once; a 4-D input gives one sequence per clip; images skip pool and newline
        b = _connector(cfg, sd, mode, out_dtype=torch.bfloat16)(feats.to(dev))
        assert b.dtype == torch.bfloat16 and ((b.double().cpu() - ref["want"]).abs() - BF16_ROUND * ref["want"].abs()).max().item() <= MARGIN * floor
        clips = m(torch.stack([feats, feats.flip(0)]).to(dev))
        assert len(clips) == 2 and torch.equal(clips[0], out) and clips[1].shape == out.shape and not torch.equal(clips[1], out)
        img = m(feats.to(dev), modality="image").cpu()
        flat = dict(cfg, mm_patch_merge_type="flat", mm_spatial_pool_stride=1)
        want_img = CO.forward(sd, flat, feats)
        fl = fp32_floor(CO.forward(sd, flat, feats, dtype=torch.float32, bf16_operands=FLOOR_OPERANDS[mode]), want_img)
        assert img.shape == want_img.shape == (CO.FRAMES * 25, CO.D_OUT) and maxabs(img, want_img) <= MARGIN * fl


# ------------------------------------------------------------------------------------------------
# 3. full width: the real tile dispatch at K = 3584 and the 56-row layout of a 7 x 7 grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_full_width_once(mode):
    dev = gpu_device()
    cfg = CO.make_config("mlp2x_gelu", "bilinear", "grid", d_in=768, d_out=3584)
    if "full.sd" not in _REFS:
        _REFS["full.sd"] = CO.make_weights("mlp2x_gelu", 1931, 768, 3584)
        _REFS["full.x"] = CO.make_features(1932, 2, 14, 768)
    sd, feats = _REFS["full.sd"], _REFS["full.x"]
    ref = _reference(sd, cfg, feats, "full")
    m = _connector(cfg, sd, mode)
    got = m(feats.to(dev)).cpu()
    assert got.shape == (2 * 7 * 8, 3584) == (m.num_tokens(2, 14), 3584)
    err, floor = maxabs(got, ref["want"]), ref["floor"][mode]
    print(f"[connector full width {mode}] vs fp64 {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}")
    assert err <= MARGIN * floor, (err, floor)
    if mode == "fp32":
        assert err <= 1e-3
    assert torch.equal(got[7], sd["image_newline"]) and torch.equal(got[-1], sd["image_newline"])


# ------------------------------------------------------------------------------------------------
# 4. frames one at a time against the same frames in one call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["mlp_bil_p5_grid", "mlp_max_p5_none", "lin_avg_p5_none"])
def test_frames_one_at_a_time(name, mode):
    dev = gpu_device()
    sd, cfg, _, _ = CO.golden_case(_gold(), name)
    feats = CO.make_features(1940, 3, 5)
    ref = _reference(sd, cfg, feats, ("seq", name))
    m = _connector(cfg, sd, mode)
    whole = m(feats.to(dev)).cpu()
    single = torch.cat([m(feats[i:i + 1].to(dev)) for i in range(3)]).cpu()          # grid / no_token: per-frame sequences concatenate
    assert whole.shape == single.shape == ref["want"].shape
    for what, got in (("one call", whole), ("frame by frame", single)):
        err = maxabs(got, ref["want"])
        print(f"[connector {name} {mode} {what}] vs fp64 {err:.3e}  floor {ref['floor'][mode]:.3e}  ratio {err / ref['floor'][mode]:.2f}")
        assert err <= MARGIN * ref["floor"][mode]


# ------------------------------------------------------------------------------------------------
# 5. StreamingVideoTokens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newline", ["grid", "one_token", "frame"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_streaming_video_tokens(mode, newline, monkeypatch):
    """Five one-frame pushes into a window of three.  The tower runs in its accurate mode; `mode` is the connector's.

    Every window is held twice:
      - against the connector oracle on the NATIVE tower's window x_t, to MARGIN times the mode's floor on that input and nothing more: the
        ring, the window's layout and the per-frame projection are bounded as a single connector call is, whatever the tower's own error;
      - against the connector oracle on the ORACLE tower's window x_o, to MARGIN * floor(x_o) plus `carried`, what the tower's distance
        from its oracle becomes behind an exact connector, max |oracle64(x_t) - oracle64(x_o)| (the triangle inequality).  The tower is not
        under test here; its window is held to tests/test_hip_parity.py's ACC_CEIL.  DESIGN.md 3.9 states this allowance."""
    import streamformer_amd as sa
    import streamformer_amd._native as nat
    from oracle import streamformer_oracle as O
    from streamformer_amd.init_weights import make_state_dict
    dev = gpu_device()
    ecfg = small_cfg(num_frames=8)                      # 48 / 16: a 3 x 3 grid, bilinear stride 2 -> 2 x 2
    esd = make_state_dict(ecfg, seed=19)
    enc = sa.TimesformerMultiTaskingModelSigLIP(ecfg, compute_dtype="fp32")
    enc.load_state_dict(esd)
    tower = sa.TimesformerVisionTower(enc.to(dev).eval(), streaming_mode=True, context_length=3)
    cfg = CO.make_config("mlp2x_gelu", "bilinear", newline, d_in=ecfg.hidden_size, d_out=192)
    sd = CO.make_weights("mlp2x_gelu", 1951, ecfg.hidden_size, 192)
    conn = _connector(cfg, sd, mode)
    stream = sa.StreamingVideoTokens(tower, conn)
    calls = []
    real = nat.lib.sf_connector_forward

    def counting(handle, feats, F, P, *rest):
        calls.append((F, P))
        return real(handle, feats, F, P, *rest)
    monkeypatch.setattr(nat.lib, "sf_connector_forward", counting)
    x = frames(19, (1, 5, 3, 48, 48))
    for round_ in range(2):
        ocache, window = O.new_cache(ecfg), None
        for t in range(5):
            got = stream.push(x[:, t:t + 1].to(dev)).cpu()
            lhs = O.forward(esd, ecfg, x[:, t:t + 1], cache=ocache)["last_hidden_state"]
            window = lhs if window is None else torch.cat([window, lhs], dim=1)[:, -3:]
            held = min(t + 1, 3)
            assert stream.frames_held == held and got.shape == (conn.num_tokens(held, 3), 192)
            want = CO.forward(sd, cfg, window[0])
            floor = fp32_floor(CO.forward(sd, cfg, window[0], dtype=torch.float32, bf16_operands=FLOOR_OPERANDS[mode]), want)
            native_window = tower.hidden_states[0].cpu()
            want_own = CO.forward(sd, cfg, native_window)
            floor_own = fp32_floor(CO.forward(sd, cfg, native_window, dtype=torch.float32, bf16_operands=FLOOR_OPERANDS[mode]), want_own)
            err_own, err = maxabs(got, want_own), maxabs(got, want)
            print(f"[streaming tokens {mode} {newline} push {t}] on the native tower's window {err_own:.3e}  floor {floor_own:.3e}  ratio "
                  f"{err_own / floor_own:.2f}   on the oracle tower's window {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}   "
                  f"tower vs its oracle {maxabs(native_window, window[0]):.3e}  behind an exact connector {maxabs(want_own, want):.3e}")
            assert err_own <= MARGIN * floor_own, (t, err_own, floor_own)
            assert maxabs(native_window, window[0]) <= 5e-4
            assert err <= MARGIN * floor + maxabs(want_own, want), (t, err, floor)
            assert torch.equal(got[-1], sd["image_newline"])
        assert calls == [(1, 3)] * 5 * (round_ + 1), "every push must project the one new frame only"
        stream.clear()                                  # restarts the stream: the second round repeats the first
        assert stream.frames_held == 0 and tower.past_key_values is None


# ------------------------------------------------------------------------------------------------
# 6. refusals leave the error set and the output untouched
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    import streamformer_amd._native as nat
    dev = gpu_device()
    sd, cfg, feats, _ = CO.golden_case(_gold(), "mlp_bil_p5_grid")
    m = _connector(cfg, sd, "fp32")
    key = m._video_key()
    h = m._handle(key)
    x = feats.to(dev).contiguous()
    n = C.c_size_t()
    nat.check(nat.lib.sf_connector_workspace_bytes(h, 2, 5, C.byref(n)))
    ws = torch.empty(n.value + 512, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) & ~255
    out = torch.full((m.num_tokens(2, 5) + 1, CO.D_OUT), float("nan"), device=dev)
    s = nat.current_stream_handle(dev)
    for what, args, code, word in (
            ("misaligned workspace", (x.data_ptr(), 2, 5, out.data_ptr(), nat.SF_F32, base + 16, n.value), nat.SF_ERR_INVALID, b"aligned"),
            ("workspace one byte short", (x.data_ptr(), 2, 5, out.data_ptr(), nat.SF_F32, base, n.value - 1), nat.SF_ERR_WORKSPACE, b"workspace"),
            ("P = 0", (x.data_ptr(), 2, 0, out.data_ptr(), nat.SF_F32, base, n.value), nat.SF_ERR_INVALID, b"patches"),
            ("bad out_dtype", (x.data_ptr(), 2, 5, out.data_ptr(), nat.SF_F64, base, n.value), nat.SF_ERR_INVALID, b"out_dtype")):
        assert nat.lib.sf_connector_forward(h, *args, s) == code, what
        assert word in nat.lib.sf_last_error(), (what, nat.lib.sf_last_error())
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), what
    # a grid connector without image_newline never finalizes, and never launches
    raw = C.c_void_p()
    nat.check(nat.lib.sf_connector_create(C.byref(nat.SfConnectorConfig(CO.D_IN, CO.D_OUT, 2, 3, 2, 3)), 0, C.byref(raw)))
    try:
        for k, v in sd.items():
            if k != "image_newline":
                shape = (C.c_int64 * v.dim())(*v.shape)
                nat.check(nat.lib.sf_connector_load_tensor(raw, k.encode(), v.data_ptr(), nat.SF_F32, shape, v.dim()))
        assert nat.lib.sf_connector_finalize(raw, nat.SF_COMPUTE_BF16X3) == nat.SF_ERR_STATE and b"image_newline" in nat.lib.sf_last_error()
        assert nat.lib.sf_connector_forward(raw, x.data_ptr(), 2, 5, out.data_ptr(), nat.SF_F32, base, n.value, s) == nat.SF_ERR_STATE
        assert b"finalize" in nat.lib.sf_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    finally:
        nat.lib.sf_connector_destroy(raw)
    # and the good call still works afterwards
    nat.check(nat.lib.sf_connector_forward(h, x.data_ptr(), 2, 5, out.data_ptr(), nat.SF_F32, base, n.value, s))
    torch.cuda.synchronize()
    assert not torch.isnan(out[:-1]).any() and torch.isnan(out[-1]).all()
