"""The Mask2Former masked-attention decoder on the MI355X: its two new kernels alone against fp64 torch over the shapes and masks at which
they take another path, and both module classes in both compute modes against the fp64 restatement of the reference
(tests/mask_decoder_oracle.py, which reproduces fixture F24).

Tolerances follow tests/test_pixel_decoder.py: each bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds, the error, against
fp64, of the same operator sequence in torch on the same inputs at the operand precision of the mode under test (plain fp32 for the two
kernels; bf16_operands="x3" / True on every Linear), and never less than one fp32 rounding of the result.  The floor is computed here, on
the CPU, from the inputs; never from the code under test.

A flipped mask bit changes everything downstream, so the module comparison is teacher-forced: the forward exports every layer's packed
mask, the oracle runs under those masks, each exported mask must equal the oracle's own threshold wherever the fp64 logit lies outside
the band (4 x the floor of that layer's logits; a cleared row is accepted if its decided bits are all hidden or all visible), at most
CAP = 5 % of a layer's bits may lie inside the band (tests/test_mask_decoder_cpu.py shows the fixture stays under half of that), and
every output is compared with the forced oracle against its floor.

Measured on an MI355X (largest error / bound per group): attention kernel 0.59 (skip and no-skip runs bit-identical), with pitches and
planes 0.17; mask kernel's pred_masks 0.24, every decided bit equal and boxes exact; module 0.31 in fp32 mode (undecided bits 0, and 0
bits differing from F24's stored masks) and 0.33 in bf16 mode (undecided bits at most 2.6 % of a layer, no decided bit differing)
(DESIGN.md section 3.15).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mask_decoder_oracle as DO
from tests.helpers import EPS32, MARGIN, check_against_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream, draw as _draw

pytestmark = pytest.mark.gpu

MODES = {"fp32": "x3", "bf16": True}
CAP = 0.05


# ------------------------------------------------------------------------------------------------
# 1. masked attention alone
# ------------------------------------------------------------------------------------------------
MASKS = ("none", "all", "first", "last", "tile", "tile15", "random")


def _mask(kind, rs, Fr, Q, HW):
    m = np.zeros((Fr, Q, HW), bool)
    if kind == "all":
        m[:] = True
    elif kind in ("first", "last"):
        m[:] = True
        m[:, :, 0 if kind == "first" else HW - 1] = False
    elif kind in ("tile", "tile15"):          # a middle 16-key tile hidden from the first 16 queries (from 15 of them)
        k0 = 16 if HW >= 33 else 0
        m[:, :16, k0:k0 + 16] = True
        if kind == "tile15":
            m[:, min(7, Q - 1), k0:k0 + 16] = False
    elif kind == "random":
        m = rs.random_sample((Fr, Q, HW)) < 0.9
    return m


def _attention_ref(q, k, v, kpos, mask, heads):
    Fr, Q, D = q.shape
    hd = D // heads
    split = lambda t: t.reshape(Fr, -1, heads, hd).transpose(1, 2)      # noqa: E731
    s = split(q) @ split(k + kpos).transpose(-1, -2) / (hd ** 0.5)
    s = s.masked_fill(torch.from_numpy(mask)[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)                  # a query without a visible key: zeros
    return (p @ split(v)).transpose(1, 2).reshape(Fr, Q, D)


@pytest.mark.parametrize("Fr", [1, 3])
@pytest.mark.parametrize("hd", [8, 32, 72, 128])
def test_attention_kernel(hd, Fr):
    nat, dev, heads = _nat(), gpu_device(), 2
    D = heads * hd
    worst = 0.0
    for Q in (1, 16, 17, 100):
        for HW in (1, 6, 31, 32, 33, 49, 65, 784):
            rs = np.random.RandomState(1000 * hd + 10 * Q + HW)
            q, k, v, kpos = _draw(rs, Fr, Q, D), _draw(rs, Fr, HW, D), _draw(rs, Fr, HW, D), _draw(rs, HW, D)
            qd, kd, vd, pd = (t.to(dev) for t in (q, k, v, kpos))
            for kind in MASKS:
                m = _mask(kind, rs, Fr, Q, HW)
                md = torch.from_numpy(DO.pack_mask(m)).to(dev)
                outs = []
                for no_skip in (0, 1):
                    buf, out = guarded(dev, Fr, Q, D)
                    nat.check(nat.lib.sf_op_maskdec_attention(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, pd.data_ptr(), D,
                                                              None if kind == "none" and no_skip else md.data_ptr(), out.data_ptr(), None, None,
                                                              Fr, Q, HW, heads, hd, no_skip, _stream()))
                    outs.append(read_guarded(buf, out))
                assert torch.equal(outs[0], outs[1]), ("skip path differs", Q, HW, kind)
                want = _attention_ref(q.double(), k.double(), v.double(), kpos.double(), m, heads)
                floor = _attention_ref(q, k, v, kpos, m, heads)
                bound = MARGIN * max(maxabs(floor, want), EPS32 * float(want.abs().max()), EPS32)
                err = maxabs(outs[0], want)
                worst = max(worst, err / bound)
                assert err <= bound, (Q, HW, kind, err, bound)
                if kind == "all":
                    assert not outs[0].any()
    print(f"  attention hd {hd} F {Fr}: largest error / bound {worst:.3f}")


def test_attention_kernel_pitches_and_planes():
    """K and V as column ranges of one [rows, 2 D] GEMM output, q of a [rows, 3 D] one, and the bf16 plane outputs."""
    nat, dev, heads, hd, Fr, Q, HW = _nat(), gpu_device(), 4, 16, 2, 20, 40
    D = heads * hd
    rs = np.random.RandomState(7)
    qb, kvb, kpos = _draw(rs, Fr, Q, 3 * D), _draw(rs, Fr, HW, 2 * D), _draw(rs, HW, D)
    m = _mask("random", rs, Fr, Q, HW)
    qd, kvd, pd, md = qb.to(dev), kvb.to(dev), kpos.to(dev), torch.from_numpy(DO.pack_mask(m)).to(dev)
    buf, out = guarded(dev, Fr, Q, D)
    hi = torch.full((Fr * Q * D + 64,), -1, dtype=torch.int16, device=dev)
    lo = torch.full((Fr * Q * D + 64,), -1, dtype=torch.int16, device=dev)
    nat.check(nat.lib.sf_op_maskdec_attention(qd.data_ptr() + 4 * D, 3 * D, kvd.data_ptr(), kvd.data_ptr() + 4 * D, 2 * D, pd.data_ptr(), D, md.data_ptr(),
                                              out.data_ptr(), hi.data_ptr(), lo.data_ptr(), Fr, Q, HW, heads, hd, 0, _stream()))
    got = read_guarded(buf, out)
    q, k, v = qb[..., D:2 * D], kvb[..., :D], kvb[..., D:]
    want = _attention_ref(q.double(), k.double(), v.double(), kpos.double(), m, heads)
    check_against_floor("attention with pitches", got, _attention_ref(q, k, v, kpos, m, heads), want)
    h, l = hi.cpu(), lo.cpu()
    assert (h[Fr * Q * D:] == -1).all() and (l[Fr * Q * D:] == -1).all()
    gh = got.flatten().to(torch.bfloat16)
    assert torch.equal(h[:Fr * Q * D], gh.view(torch.int16))
    assert torch.equal(l[:Fr * Q * D], (got.flatten() - gh.float()).to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------------------------------------
# 2. mask logits -> packed mask / masks + boxes
# ------------------------------------------------------------------------------------------------
def _accept_masks(what, got, raw, low, band):
    """got, raw: bool [F, Q, P] (the kernel's mask; the fp64 threshold BEFORE the clearing rule); low: fp64 logits.  Outside the band the
    bits agree with the reference's rule; a cleared row is accepted if its decided bits are all hidden or all visible."""
    decided = low.abs() > band
    share = 1.0 - float(decided.double().mean())
    assert share <= CAP, (what, "undecided share", share)
    bad = 0
    for f in range(got.shape[0]):
        for q in range(got.shape[1]):
            d, g, r = decided[f, q], got[f, q], raw[f, q]
            if not g.any() and (r[d].all() or not r[d].any()):
                continue                     # cleared (or visible everywhere)
            assert g.any() or not d.any(), (what, f, q, "row cleared although decided bits differ")
            bad += int((g[d] != r[d]).sum())
    assert bad == 0, (what, "decided bits differ", bad)
    return share


@pytest.mark.parametrize("Q", [1, 33, 100])
@pytest.mark.parametrize("HWhw", [((8, 8), (2, 2)), ((12, 20), (3, 5)), ((7, 9), (7, 9)), ((56, 56), (7, 7))])
def test_mask_kernel(HWhw, Q):
    nat, dev, Fr, Dm = _nat(), gpu_device(), 2, 64
    (H, W), (h, w) = HWhw
    rs = np.random.RandomState(H * 100 + Q)
    me, mf = _draw(rs, Fr, Q, Dm), _draw(rs, Fr, Dm, H, W)
    # constructed rows: channel 0 of the features marks the source block of low-resolution pixel (0, 0), channel 1 is constant one
    mf[:, 0] = 0.0
    mf[:, 0, :H // h, :W // w] = 1.0
    mf[:, 1] = 1.0
    me[:, :, 0] = 0.0
    me[:, 0, 1] = -100.0                     # row 0: below zero everywhere -> comes back cleared
    if Q > 1:
        me[:, 1, 1] = 100.0                  # row 1: above zero everywhere
    if Q > 2:
        me[:, 2, 1], me[:, 2, 0] = -100.0, 200.0      # row 2: below zero except one pixel
    med, mfd = me.to(dev), mf.to(dev)
    words = (h * w + 31) // 32
    bits = torch.full((Fr * Q * words + 64,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    lbuf, logits = guarded(dev, Fr, Q, H, W)
    bbuf, boxes = guarded(dev, Fr, Q, 4)
    ws = torch.empty(nat.lib.sf_op_maskdec_mask_workspace_bytes(Fr, Dm, h, w), dtype=torch.uint8, device=dev)
    nat.check(nat.lib.sf_op_maskdec_mask(med.data_ptr(), mfd.data_ptr(), Fr, Q, Dm, H, W, h, w, bits.data_ptr(), logits.data_ptr(), boxes.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()))
    host = bits.cpu()
    assert (host[Fr * Q * words:] == 0x5a5a5a5a).all(), "the guard words were written"
    got = torch.from_numpy(DO.unpack_mask(host[:Fr * Q * words].view(Fr, Q, words).numpy(), h * w))
    full64 = torch.einsum("bqc,bchw->bqhw", me.double(), mf.double())
    low64 = F.interpolate(full64, size=(h, w), mode="bilinear", align_corners=False).flatten(2)
    low32 = torch.einsum("bqc,bchw->bqhw", me, F.interpolate(mf, size=(h, w), mode="bilinear", align_corners=False)).flatten(2)      # the kernel's order
    band = MARGIN * max(maxabs(low32, low64), EPS32 * float(low64.abs().max()))
    raw = low64 < 0
    share = _accept_masks("mask kernel", got, raw, low64, band)
    assert raw[:, 0].all() and not got[:, 0].any()
    if Q > 1:
        assert not raw[:, 1].any() and not got[:, 1].any()
    if Q > 2:
        assert int((~raw[:, 2]).sum()) == Fr and torch.equal(got[:, 2], raw[:, 2]) and not got[:, 2, 0].any()
    # the last layer's variant: masks at full resolution and boxes
    pm = read_guarded(lbuf, logits)
    check_against_floor(f"pred_masks {H}x{W} Q {Q} (undecided {share:.4f})", pm, torch.einsum("bqc,bchw->bqhw", me, mf), full64)
    fband = MARGIN * max(maxabs(torch.einsum("bqc,bchw->bqhw", me, mf), full64), EPS32 * float(full64.abs().max()))
    bx = read_guarded(bbuf, boxes)
    sure = ~(full64.abs() <= fband).flatten(2).any(-1)
    assert sure.double().mean() > 0.5
    assert torch.equal(bx[sure], DO.boxes_of(full64)[sure])
    assert not bx[:, 0].any()                # no pixel above zero: zeros


# ------------------------------------------------------------------------------------------------
# 3. the modules
# ------------------------------------------------------------------------------------------------
def _module(c, mode):
    import streamformer_amd as sa
    m = getattr(sa, c["cls"])(c["in_channels"], **dict(DO.decoder_kwargs(c), compute_dtype=mode)).eval()
    m.load_state_dict(DO.make_weights(c), strict=True)
    return m.to(gpu_device())


@functools.lru_cache(maxsize=None)
def _golden():
    return DO.load_golden()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(DO.CASES))
def test_module(name, mode):
    c, dev = DO.CASES[name], gpu_device()
    sd = DO.make_weights(c)
    xs, mf = DO.make_inputs(c)
    m = _module(c, mode)
    xd, mfd = [x.to(dev) for x in xs], mf.to(dev)
    out = m(xd, mfd, return_attn_masks=True, return_aux=True)
    torch.cuda.synchronize()
    masks = [t.cpu() for t in out["attn_masks"]]
    assert len(masks) == c["layers"] and len(out["aux_outputs"]) == c["layers"]
    want = DO.forward(sd, c, xs, mf, table="fp64", masks=masks)
    floor = DO.forward(sd, c, xs, mf, dtype=torch.float32, operands=MODES[mode], table="fp64", masks=masks, interp="features")
    for i, packed in enumerate(masks):
        low = want["low_logits"][i]
        band = MARGIN * max(maxabs(floor["low_logits"][i], low), EPS32 * float(low.abs().max()))
        got = torch.from_numpy(DO.unpack_mask(packed.numpy(), low.shape[-1]))
        share = _accept_masks(f"{name} {mode} layer {i}", got, low < 0, low, band)
        line = f"  {name} {mode} layer {i}: band {band:.3e}, undecided {share:.4f}"
        if mode == "fp32":
            line += f", bits differing from F24: {int((DO.unpack_mask(_golden()[f'{name}.attn_mask{i}'], low.shape[-1]) != got.numpy()).sum())}"
        print(line)
    keys = [k for k in DO.OUTPUTS if k in want and k != "pred_bboxes"]
    assert keys == [k for k in DO.OUTPUTS if k in out and k != "pred_bboxes"]
    for k in keys:
        assert out[k].shape == want[k].shape
        check_against_floor(f"{name} {mode} {k}", out[k], floor[k], want[k])
    if DO.is_cl(c):
        pm = want["pred_masks"]
        fband = MARGIN * max(maxabs(floor["pred_masks"], pm), EPS32 * float(pm.abs().max()))
        sure = ~(pm.abs() <= fband).flatten(2).any(-1)
        assert sure.any() and torch.equal(out["pred_bboxes"].cpu()[sure], want["pred_bboxes"][sure])
        assert torch.equal(out["query_pos_embeds"].cpu(), sd["query_embed.weight"][None].expand(mf.shape[0], -1, -1))
    # the last-but-one prediction (the last aux entry) against the forced oracle
    for k, v in out["aux_outputs"][-1].items():
        check_against_floor(f"{name} {mode} aux[-1].{k}", v, floor["aux"][-1][k], want["aux"][-1][k])
    # two calls are bit-identical, aux_outputs is empty unless asked for, and a side stream gives the same bits
    again = m(xd, mfd)
    assert again["aux_outputs"] == [] and "attn_masks" not in again
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = m(xd, mfd)
    side.synchronize()
    for k in keys + (["pred_bboxes"] if DO.is_cl(c) else []):
        assert torch.equal(again[k], out[k]) and torch.equal(other[k], out[k]), k


def test_chain_from_the_pixel_decoder():
    """MSDeformAttnPixelDecoder.forward_features' outputs go into the decoder as they are: the same bits as from copies."""
    import streamformer_amd as sa
    from tests import pixel_decoder_oracle as PO
    dev = gpu_device()
    pc = PO.CASES["m2f"]
    pix = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, pc["channels"], PO.STRIDES)}, **PO.decoder_kwargs(pc)).eval()
    pix.load_state_dict(PO.make_weights(pc), strict=True)
    pix = pix.to(dev)
    c = dict(DO.CASES["cl"], in_channels=pc["conv_dim"], mask_dim=pc["mask_dim"])
    dec = _module_from(c)
    mask_features, _, ms = pix.forward_features({k: v.to(dev) for k, v in PO.make_features(pc).items()})
    a = dec(ms, mask_features)
    b = dec([t.clone() for t in ms], mask_features.clone())
    for k in DO.OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all(), k
    assert a["pred_masks"].shape == (mask_features.shape[0], c["queries"]) + tuple(mask_features.shape[2:])


def _module_from(c):
    import streamformer_amd as sa
    m = getattr(sa, c["cls"])(c["in_channels"], **DO.decoder_kwargs(c)).eval()
    m.load_state_dict(DO.make_weights(c), strict=True)
    return m.to(gpu_device())
