"""The Mask2Former pixel decoder on the MI355X: each of its kernels alone against fp64 torch over the shapes at which it takes another
path, and the whole module in both compute modes against the fp64 restatement of the reference (tests/pixel_decoder_oracle.py, which
reproduces fixture F23).

Tolerances follow tests/test_msda.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds — the error, against fp64, of
the same operator sequence in torch on the same inputs at the operand precision of the mode under test (plain fp32 for the streaming
kernels; bf16_operands="x3" / True on every GEMM) — and never less than one fp32 rounding of the result.  The floor is computed here, on
the CPU, from the inputs; never from the code under test.  Plane outputs (bf16 hi / lo bit patterns) are compared as bits against the
split rule hi = bf16(x), lo = bf16(x - hi).

Measured on an MI355X (largest error / bound per group): layout moves bit-exact; GroupNorm 0.49, with upsample 0.32; position table 0.08,
reference points 0.10; post-LN 0.33; 3 x 3 gather + GEMM 0.25; module 0.31 in fp32 mode and 0.26 in bf16 mode.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_decoder_oracle as PO
from tests import vit_adapter_oracle as VO
from tests.helpers import bf16_bits, check_against_floor, gpu_device, guarded, read_guarded
from tests.helpers import native as _nat, stream as _stream, draw as _draw
from tests.oracle_ops import layernorm, operand_linear

pytestmark = pytest.mark.gpu

MODES = {"fp32": "x3", "bf16": True}
FRAMES = 2
SENTINEL = -1            # 0xffff: a bf16 NaN no kernel writes


def guarded_bits(dev, *shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.int16, device=dev)
    return buf, buf[:n].view(*shape)


def read_guarded_bits(buf, view):
    host = buf.cpu()
    assert (host[view.numel():] == SENTINEL).all(), "the guard row was written"
    assert not (host[:view.numel()] == SENTINEL).any(), "plane elements left unwritten"
    return host[:view.numel()].view(view.shape)


def split_bits(x):
    """The operand split of a compute mode: hi = bf16(x), lo = bf16(x - hi), as bit patterns."""
    hi = x.to(torch.bfloat16)
    return hi.view(torch.int16), bf16_bits(x - hi.float())


def planes_value(hi, lo=None):
    v = hi.view(torch.bfloat16).float()
    return v if lo is None else v + lo.view(torch.bfloat16).float()


def rows_of(x):
    return x.flatten(2).transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------
# 1. NCHW -> planes and rows -> NCHW
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 6, 49, 65, 240])
@pytest.mark.parametrize("C_", [8, 64, 72, 192])
def test_layout_moves(C_, HW):
    nat, dev = _nat(), gpu_device()
    x = _draw(np.random.RandomState(2700 + C_ + HW), FRAMES, C_, HW)
    xd = x.to(dev)
    bh, hi = guarded_bits(dev, FRAMES * HW, C_)
    bl, lo = guarded_bits(dev, FRAMES * HW, C_)
    nat.check(nat.lib.sf_op_pixdec_nchw_to_planes(xd.data_ptr(), hi.data_ptr(), lo.data_ptr(), FRAMES, C_, HW, _stream()))
    torch.cuda.synchronize()
    hi_h, lo_h = read_guarded_bits(bh, hi), read_guarded_bits(bl, lo)
    want_hi, want_lo = split_bits(rows_of(x.view(FRAMES, C_, HW, 1)).reshape(FRAMES * HW, C_))
    assert torch.equal(hi_h, want_hi) and torch.equal(lo_h, want_lo)
    # without a lo plane the hi plane is the same
    bh2, hi2 = guarded_bits(dev, FRAMES * HW, C_)
    nat.check(nat.lib.sf_op_pixdec_nchw_to_planes(xd.data_ptr(), hi2.data_ptr(), None, FRAMES, C_, HW, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(read_guarded_bits(bh2, hi2), want_hi)
    # rows -> NCHW is a pure move, also out of longer frames (a level's slice of [F, S, C])
    pad = 3
    rows = torch.full((FRAMES, HW + pad, C_), float("nan"))
    rows[:, 1:1 + HW] = rows_of(x.view(FRAMES, C_, HW, 1))
    rd = rows.to(dev)
    bo, out = guarded(dev, FRAMES, C_, HW)
    nat.check(nat.lib.sf_op_pixdec_rows_to_nchw(rd.data_ptr() + 4 * C_, (HW + pad) * C_, out.data_ptr(), FRAMES, C_, HW, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(read_guarded(bo, out), x)
    # round trip through both: exact in the hi + lo sum to 2^-16 relative
    back = planes_value(hi_h, lo_h).view(FRAMES, HW, C_).to(dev).contiguous()
    bo, out = guarded(dev, FRAMES, C_, HW)
    nat.check(nat.lib.sf_op_pixdec_rows_to_nchw(back.data_ptr(), HW * C_, out.data_ptr(), FRAMES, C_, HW, _stream()))
    torch.cuda.synchronize()
    got = read_guarded(bo, out)
    assert bool(((got - x).abs() <= 2.0 ** -16 * x.abs()).all())


# ------------------------------------------------------------------------------------------------
# 2. GroupNorm, every apply variant
# ------------------------------------------------------------------------------------------------
def _op_groupnorm(x, gamma, beta, relu=False, prev=None, pos=None):
    """x NCHW, prev NCHW or None, pos [HW, C] or None -> (y NCHW, y_hi, y_lo, q_hi, q_lo) as the kernel wrote them."""
    nat, dev = _nat(), gpu_device()
    Fr, C_, H, W = x.shape
    xd, gd, bd = rows_of(x).to(dev), gamma.to(dev), beta.to(dev)
    pd = rows_of(prev).to(dev) if prev is not None else None
    posd = pos.to(dev).contiguous() if pos is not None else None
    stats = torch.empty(Fr * 32 * 4, device=dev)
    by, y = guarded(dev, Fr, H * W, C_)
    planes = [guarded_bits(dev, Fr * H * W, C_) for _ in range(4 if pos is not None else 2)]
    ptrs = [v.data_ptr() for _, v in planes] + [None] * (4 - len(planes))
    Hp, Wp = (prev.shape[2], prev.shape[3]) if prev is not None else (0, 0)
    nat.check(nat.lib.sf_op_pixdec_groupnorm(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), int(relu), nat.ptr(pd), Hp, Wp, nat.ptr(posd),
                                             stats.data_ptr(), y.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], Fr, H, W, C_, _stream()))
    torch.cuda.synchronize()
    yh = read_guarded(by, y)
    return (yh.transpose(1, 2).reshape(Fr, C_, H, W), yh.reshape(-1, C_)) + tuple(read_guarded_bits(b, v) for b, v in planes)


def _gn_sides(x, gamma, beta, relu, prev):
    def run(dt):
        y = F.group_norm(x.to(dt), 32, gamma.to(dt), beta.to(dt), PO.GN_EPS)
        if relu:
            y = torch.relu(y)
        if prev is not None:
            y = y + F.interpolate(prev.to(dt), size=x.shape[-2:], mode="bilinear", align_corners=False)
        return y
    return run(torch.float64), run(torch.float32)


def _gn_drawings(rs, C_, H, W):
    base = _draw(rs, FRAMES, C_, H, W)
    sign = 1.0 - 2.0 * (torch.arange(32) % 2)
    offset = base + 100.0 * sign.repeat_interleave(C_ // 32)[None, :, None, None]      # per group +-100 at unit spread: mean^2 / variance = 1e4
    scaled = base.clone()
    scaled[1] = scaled[0] * 1000.0            # statistics leaking across frames show at once
    return {"normal": base, "offset100": offset, "frame1=1000*frame0": scaled}


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (12, 20)])
@pytest.mark.parametrize("C_", [64, 128])
def test_groupnorm_plain_and_relu(C_, H, W):
    rs = np.random.RandomState(2710 + C_ + 7 * H + W)
    gamma, beta = 1.0 + 0.1 * _draw(rs, C_), 0.1 * _draw(rs, C_)
    pos = _draw(rs, H * W, C_)
    for name, x in _gn_drawings(rs, C_, H, W).items():
        for relu in (False, True):
            want, floor = _gn_sides(x, gamma, beta, relu, None)
            y, y_rows, y_hi, y_lo, q_hi, q_lo = _op_groupnorm(x, gamma, beta, relu, None, pos)
            check_against_floor(f"groupnorm {H}x{W} C={C_} {name} relu={relu}", y, floor, want)
            assert (torch.equal(y_hi, split_bits(y_rows)[0]) and torch.equal(y_lo, split_bits(y_rows)[1])), "y planes are not the split of y"
            q = y_rows + pos.repeat(FRAMES, 1)
            assert torch.equal(q_hi, split_bits(q)[0]) and torch.equal(q_lo, split_bits(q)[1]), "q planes are not the split of y + pos"
            again = _op_groupnorm(x, gamma, beta, relu, None, pos)
            assert all(torch.equal(a, b) for a, b in zip(again, (y, y_rows, y_hi, y_lo, q_hi, q_lo))), "two runs differ"


@pytest.mark.parametrize("src,dst", [((2, 3), (3, 5)), ((4, 4), (7, 7)), ((1, 1), (4, 4))])
@pytest.mark.parametrize("C_", [64, 128])
def test_groupnorm_with_upsample(C_, src, dst):
    rs = np.random.RandomState(2730 + C_ + 11 * dst[0] + dst[1])
    gamma, beta = 1.0 + 0.1 * _draw(rs, C_), 0.1 * _draw(rs, C_)
    prev = _draw(rs, FRAMES, C_, *src)
    prev[1] += 1000.0                         # a corner taken from the other frame shows at once
    for name, x in _gn_drawings(rs, C_, *dst).items():
        want, floor = _gn_sides(x, gamma, beta, False, prev)
        got = _op_groupnorm(x, gamma, beta, False, prev)
        check_against_floor(f"groupnorm + upsample {src} -> {dst} C={C_} {name}", got[0], floor, want)
        assert all(torch.equal(a, b) for a, b in zip(_op_groupnorm(x, gamma, beta, False, prev), got)), "two runs differ"


# ------------------------------------------------------------------------------------------------
# 3. position table + reference points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [64, 256])
def test_position_table_and_reference_points(C_):
    nat, dev = _nat(), gpu_device()
    shapes = [(1, 1), (2, 3), (12, 20)]
    S, L = sum(h * w for h, w in shapes), len(shapes)
    le = _draw(np.random.RandomState(2750 + C_), L, C_)
    bp, pos = guarded(dev, S, C_)
    br, ref = guarded(dev, FRAMES, S, L, 2)
    c_shapes = (C.c_int32 * (2 * L))(*[d for s in shapes for d in s])
    led = le.to(dev)
    nat.check(nat.lib.sf_op_pixdec_pos_ref(led.data_ptr(), c_shapes, L, FRAMES, C_, pos.data_ptr(), ref.data_ptr(), _stream()))
    torch.cuda.synchronize()

    def table(dt, kind):
        return torch.cat([PO.to_rows(PO.position_table(h, w, C_, dt, kind)[None])[0] + le[l].to(dt) for l, (h, w) in enumerate(shapes)])

    check_against_floor(f"position table C={C_}", read_guarded(bp, pos), table(torch.float32, "as_reference"), table(torch.float64, "fp64"))
    want = PO.reference_points(shapes, torch.float64, "fp64").expand(FRAMES, -1, -1, -1)
    floor = PO.reference_points(shapes, torch.float32, "as_reference").expand(FRAMES, -1, -1, -1)
    check_against_floor("reference points", read_guarded(br, ref), floor, want)


# ------------------------------------------------------------------------------------------------
# 4. post-LN with planes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,pos_rows", [(1, 1), (5, 1), (65, 13), (2 * 86, 86)])
@pytest.mark.parametrize("C_", [4, 64, 256, 260])
def test_postln_with_planes(C_, rows, pos_rows):
    nat, dev = _nat(), gpu_device()
    rs = np.random.RandomState(2760 + C_ + rows)
    x = _draw(rs, rows, C_) + 3.0 * _draw(rs, rows, 1)
    gamma, beta, pos = 1.0 + 0.1 * _draw(rs, C_), 0.1 * _draw(rs, C_), _draw(rs, pos_rows, C_)
    xd, gd, bd, pd = x.to(dev), gamma.to(dev), beta.to(dev), pos.to(dev)

    def run(lo=True, q=True):
        by, y = guarded(dev, rows, C_)
        planes = [guarded_bits(dev, rows, C_) if asked else None for asked in (True, lo, q, q and lo)]      # y_hi, y_lo, q_hi, q_lo
        nat.check(nat.lib.sf_op_pixdec_postln(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), PO.LN_EPS, pd.data_ptr() if q else None, pos_rows if q else 0,
                                              y.data_ptr(), *[p[1].data_ptr() if p else None for p in planes], rows, C_, _stream()))
        torch.cuda.synchronize()
        return (read_guarded(by, y),) + tuple(read_guarded_bits(*p) if p else None for p in planes)

    y, y_hi, y_lo, q_hi, q_lo = run()
    check_against_floor(f"post-LN rows={rows} C={C_}", y, layernorm(x, gamma, beta, PO.LN_EPS), layernorm(x.double(), gamma.double(), beta.double(), PO.LN_EPS))
    assert torch.equal(y_hi, split_bits(y)[0]) and torch.equal(y_lo, split_bits(y)[1])
    q = y + pos.repeat(rows // pos_rows, 1)               # the pos row index wraps per frame
    assert torch.equal(q_hi, split_bits(q)[0]) and torch.equal(q_lo, split_bits(q)[1])
    full = (y, y_hi, y_lo, q_hi, q_lo)
    assert all(torch.equal(a, b) for a, b in zip(run(), full)), "two runs differ"
    for lo, q in ((False, True), (True, False), (False, False)):      # without the lo planes, without the positional addend: the rest stays
        assert all(a is None or torch.equal(a, b) for a, b in zip(run(lo, q), full)), (lo, q)


# ------------------------------------------------------------------------------------------------
# 5. 3 x 3 gather + GEMM
# ------------------------------------------------------------------------------------------------
def _op_conv3x3(x, w, mode, chunk_rows=0):
    """x NCHW, w [N, C, 3, 3] -> NCHW through planes, the gather and the GEMM."""
    nat, dev = _nat(), gpu_device()
    Fr, C_, H, W = x.shape
    N = w.shape[0]
    split = MODES[mode] == "x3"
    xh, xl = (t.to(dev) for t in split_bits(rows_of(x).reshape(-1, C_)))
    wh, wl = (t.to(dev) for t in split_bits(w.permute(0, 2, 3, 1).reshape(N, 9 * C_).contiguous()))
    ws = torch.empty(nat.lib.sf_op_pixdec_conv3x3_workspace_bytes(Fr, H, W, C_, chunk_rows), dtype=torch.uint8, device=dev)
    bo, out = guarded(dev, Fr, H * W, N)
    nat.check(nat.lib.sf_op_pixdec_conv3x3(xh.data_ptr(), xl.data_ptr() if split else None, wh.data_ptr(), wl.data_ptr() if split else None, Fr, H, W, C_, N,
                                           chunk_rows, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return read_guarded(bo, out).transpose(1, 2).reshape(Fr, N, H, W)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (12, 20)])
def test_conv3x3_vs_fp64(H, W, mode):
    C_ = N = 64
    rs = np.random.RandomState(2770 + 7 * H + W)
    x = _draw(rs, FRAMES, C_, H, W)
    w = _draw(rs, N, C_, 3, 3) / (9 * C_) ** 0.5
    lin = lambda a, b, c: operand_linear(a, b, c, MODES[mode])      # noqa: E731
    for name, inp in (("normal", x), ("constant frames", x + torch.tensor([1000.0, -3000.0])[:, None, None, None])):
        # each frame holds its own large constant: a tap that crosses a frame or wraps a row shows
        want = F.conv2d(inp.double(), w.double(), None, 1, 1)
        got = _op_conv3x3(inp, w, mode)
        check_against_floor(f"conv3x3 {H}x{W} {mode} {name}", got, PO.conv3x3(inp, w, lin), want)
        if (H, W) == (12, 20):
            # 480 pixels in chunks of 170: three chunks, a partial last one, the border 170 = 8 * 20 + 10 inside an image row
            assert torch.equal(_op_conv3x3(inp, w, mode, chunk_rows=170), got), "the chunked run differs from the single-chunk run"
            assert torch.equal(_op_conv3x3(inp, w, mode, chunk_rows=97), got), "the chunked run differs from the single-chunk run"


def test_im2col_alone():
    nat, dev = _nat(), gpu_device()
    C_, H, W = 64, 3, 5
    x = _draw(np.random.RandomState(2780), FRAMES, C_, H, W)
    hi, lo = (t.to(dev) for t in split_bits(rows_of(x).reshape(-1, C_)))
    row0, rows = 7, 19                                          # starts inside frame 0, ends inside frame 1
    bh, oh = guarded_bits(dev, rows, 9 * C_)
    bl, ol = guarded_bits(dev, rows, 9 * C_)
    nat.check(nat.lib.sf_op_pixdec_im2col(hi.data_ptr(), lo.data_ptr(), FRAMES, H, W, C_, row0, rows, oh.data_ptr(), ol.data_ptr(), _stream()))
    torch.cuda.synchronize()
    cols = F.unfold(x, 3, padding=1).view(FRAMES, C_, 9, H * W).permute(0, 3, 2, 1).reshape(FRAMES * H * W, 9 * C_)      # (dy, dx, c) order
    want_hi, want_lo = split_bits(cols[row0:row0 + rows].contiguous())
    zero = cols[row0:row0 + rows] == 0                          # padding taps: +0 in both planes
    assert torch.equal(read_guarded_bits(bh, oh), want_hi)
    assert torch.equal(torch.where(zero, torch.zeros_like(want_lo), read_guarded_bits(bl, ol)), torch.where(zero, torch.zeros_like(want_lo), want_lo))


# ------------------------------------------------------------------------------------------------
# 6. the whole module
# ------------------------------------------------------------------------------------------------
def _module(name, mode, sd=None, **kw):
    import streamformer_amd as sa
    c = PO.CASES[name]
    shape = {k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, c["channels"], PO.STRIDES)}
    m = sa.MSDeformAttnPixelDecoder(shape, compute_dtype=mode, **dict(PO.decoder_kwargs(c), **kw))
    m.load_state_dict(PO.make_weights(c) if sd is None else sd, strict=True)
    return m.to(gpu_device()).eval()


def _features(name):
    return {k: v.to(gpu_device()) for k, v in PO.make_features(PO.CASES[name]).items()}


@functools.lru_cache(maxsize=None)
def _want(name):
    c = PO.CASES[name]
    return PO.forward(PO.make_weights(c), c, PO.make_features(c), table="fp64")


@functools.lru_cache(maxsize=None)
def _floor(name, mode):
    c = PO.CASES[name]
    return PO.forward(PO.make_weights(c), c, PO.make_features(c), dtype=torch.float32, operands=MODES[mode], table="as_reference")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(PO.CASES))
def test_module_vs_fp64(name, mode):
    c = PO.CASES[name]
    m = _module(name, mode)
    feats = _features(name)
    mask, first, ms = m.forward_features(feats)
    torch.cuda.synchronize()
    assert first is ms[0] and len(ms) == 3
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in [mask] + ms)
    (want_mask, want_out), (floor_mask, floor_out) = _want(name), _floor(name, mode)
    assert mask.shape == want_mask.shape and [t.shape for t in ms] == [t.shape for t in want_out[:3]]
    check_against_floor(f"{name} {mode} mask_features", mask, floor_mask, want_mask)
    for i, t in enumerate(ms):
        check_against_floor(f"{name} {mode} out[{i}]", t, floor_out[i], want_out[i])
    again = m.forward_features(feats)
    assert torch.equal(again[0], mask) and all(torch.equal(a, b) for a, b in zip(again[2], ms)), "two forwards differ"
    # bf16-representable weights stored as fp64: load_tensor's dtype path gives the same handle
    sd16 = {k: v.to(torch.bfloat16).float() for k, v in PO.make_weights(c).items()}
    a = _module(name, mode, sd16).forward_features(feats)
    b = _module(name, mode, sd16).double()
    assert all(p.dtype == torch.float64 for p in b.parameters())
    b = b.forward_features(feats)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_module_chunked_conv_is_bit_equal():
    feats = _features("res5only")
    a = _module("res5only", "fp32").forward_features(feats)
    b = _module("res5only", "fp32", im2col_chunk_rows=97).forward_features(feats)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_module_repacks_when_a_parameter_changes():
    feats = _features("m2f")
    m = _module("m2f", "fp32")
    before = m.forward_features(feats)[0].clone()
    with torch.no_grad():
        m.mask_features.weight.mul_(1.5)
        m.transformer.encoder.layers[1].norm2.bias.add_(0.25)
    after = m.forward_features(feats)[0]
    assert not torch.equal(after, before)
    fresh = _module("m2f", "fp32", {k: v.cpu() for k, v in m.state_dict().items()})
    assert torch.equal(fresh.forward_features(feats)[0], after)


def test_module_on_the_adapter_pyramid():
    import streamformer_amd as sa
    c = VO.CASES["novit"]
    dev = gpu_device()
    backbone = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(VO.config(c), compute_dtype="fp32", **VO.adapter_kwargs(c))
    backbone.load_state_dict(VO.make_weights(c), strict=True)
    backbone = backbone.to(dev).eval()
    pyramid, _ = backbone.forward_with_tokens(VO.make_pixels(c).to(dev))
    D = c["hidden"]
    dec = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(D, s) for k, s in zip(PO.LEVELS, PO.STRIDES)}, transformer_dropout=0.0, transformer_nheads=8,
                                      transformer_dim_feedforward=128, transformer_enc_layers=2, conv_dim=64, mask_dim=64, norm="GN",
                                      transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    torch.manual_seed(2790)
    for mod in dec.modules():                 # the reference leaves these at zero: the sampling would not depend on the query
        if isinstance(mod, sa.MSDeformAttn):
            torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.2)
            torch.nn.init.normal_(mod.attention_weights.weight, std=0.2)
    dec = dec.to(dev).eval()
    mask, first, ms = dec.forward_features(pyramid)
    Fr = c["B"] * c["T"]
    Hg, Wg = VO.grid(c)
    assert mask.shape == (Fr, 64, 4 * Hg, 4 * Wg)
    assert [tuple(t.shape) for t in ms] == [(Fr, 64, Hg // 2, Wg // 2), (Fr, 64, Hg, Wg), (Fr, 64, 2 * Hg, 2 * Wg)]
    assert all(bool(torch.isfinite(t).all()) for t in [mask] + ms)
    again = dec.forward_features({k: v.clone() for k, v in pyramid.items()})
    assert torch.equal(again[0], mask) and all(torch.equal(a, b) for a, b in zip(again[2], ms))


def test_handle_refusals_write_nothing():
    nat, dev = _nat(), gpu_device()
    c = PO.CASES["m2f"]
    m = _module("m2f", "fp32")
    feats = [v.contiguous() for v in _features("m2f").values()]
    shapes = (C.c_int32 * 8)(*[d for g in c["grids"] for d in g])
    bm, mask = guarded(dev, FRAMES, c["mask_dim"], *c["grids"][0])
    outs = [guarded(dev, FRAMES, c["conv_dim"], *c["grids"][l]) for l in PO.out_levels(c)[:3]]
    fptr = (C.c_void_p * 4)(*[t.data_ptr() for t in feats])
    optr = (C.c_void_p * 3)(*[v.data_ptr() for _, v in outs])

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(b).all()) for b in [bm] + [b for b, _ in outs])

    def call(h, fp=fptr, n_levels=4, mk=None, op=optr, n_ms=3, ws=None, ws_bytes=None):
        return nat.lib.sf_pixdec_forward(h, fp, FRAMES, shapes, n_levels, mask.data_ptr() if mk is None else mk, op, n_ms,
                                         ws.data_ptr() if ws is not None else 256, ws.numel() if ws_bytes is None else ws_bytes, _stream())

    # before finalize
    raw = m._create(0)
    try:
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        assert call(raw, ws=ws) == nat.SF_ERR_STATE and untouched()
    finally:
        nat.lib.sf_pixdec_destroy(raw)
    h = m._handle()
    nbytes = C.c_size_t()
    nat.check(nat.lib.sf_pixdec_workspace_bytes(h, FRAMES, shapes, 4, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    assert call(h, ws=ws, ws_bytes=nbytes.value - 256) == nat.SF_ERR_WORKSPACE and b"workspace" in nat.lib.sf_last_error() and untouched()
    assert call(h, n_levels=3, ws=ws) == nat.SF_ERR_INVALID and b"level" in nat.lib.sf_last_error() and untouched()
    assert call(h, n_ms=2, ws=ws) == nat.SF_ERR_INVALID and untouched()
    assert call(h, mk=mask.data_ptr() + 4, ws=ws) == nat.SF_ERR_INVALID and b"aligned" in nat.lib.sf_last_error() and untouched()
    bad = (C.c_void_p * 4)(*[t.data_ptr() + (4 if i == 1 else 0) for i, t in enumerate(feats)])
    assert call(h, fp=bad, ws=ws) == nat.SF_ERR_INVALID and b"aligned" in nat.lib.sf_last_error() and untouched()
    # and the accepted call fills everything
    assert call(h, ws=ws) == 0
    torch.cuda.synchronize()
    read_guarded(bm, mask)
    for b, v in outs:
        read_guarded(b, v)
