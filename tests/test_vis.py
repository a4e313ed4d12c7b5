"""Video instance segmentation on the MI355X: the four kernels of csrc/sf_vis.hip alone against fp64 torch, SimpleTracker on the GPU against
fixture F25 (the reference's own tracker and inference_video; tests/vis_oracle.py restates them), and VideoInstanceSegmenter's wiring.

Tolerances follow tests/test_mask_decoder.py: a bound is MARGIN = 4 times the PRECISION FLOOR of what it bounds (the error, against fp64,
of the same operator sequence in fp32 torch on the CPU, and never less than one fp32 rounding of the result), computed here from the
inputs and never from the code under test.  A thresholded bit is compared where it is DECIDED: where the fp64 logit lies outside the
band of 4 x floor; at most CAP = 1 % of the bits may lie inside (tests/test_vis_cpu.py shows the cases stay under it by the reference
alone).  Discrete outputs of the tracker are compared exactly: F25's smallest decision margin is 1e-3 relative.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vis_oracle as VO
from tests.helpers import EPS32, MARGIN, check_against_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream, guarded_ints as _ints, read_guarded_ints as _read_ints

pytestmark = pytest.mark.gpu
CAP = 0.01


# ------------------------------------------------------------------------------------------------
# a. scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 2), (3, 17, 6), (2, 100, 41)])
def test_scores_kernel(shape):
    nat, dev = _nat(), gpu_device()
    Fr, Q, C1 = shape
    x = torch.from_numpy(np.random.RandomState(C1).standard_normal(shape).astype(np.float32)) * 3
    if Q > 1:
        x[0, 1, :2] = x[0, 1].max() + 1.0                   # a tie of the two best classes: the first index wins
    rows = Fr * Q
    mbuf, mx = guarded(dev, Fr, Q)
    sbuf, sc = guarded(dev, Fr, Q, C1 - 1)
    lab = _ints(dev, rows)
    xd = x.to(dev)
    for full in (False, True):
        nat.check(nat.lib.sf_op_vis_scores(xd.data_ptr(), rows, C1, mx.data_ptr(), lab.data_ptr(), sc.data_ptr() if full else None, _stream()))
    want = F.softmax(x.double(), -1)[..., :-1]
    floor = F.softmax(x, -1)[..., :-1]
    check_against_floor(f"scores {shape}", read_guarded(sbuf, sc), floor, want)
    check_against_floor(f"max scores {shape}", read_guarded(mbuf, mx), floor.max(-1)[0], want.max(-1)[0])
    labels = _read_ints(lab, rows).view(Fr, Q).long()
    band = MARGIN * max(maxabs(floor, want), EPS32 * float(want.abs().max()))
    top = torch.sort(want, -1, descending=True)[0]
    decided = (top[..., 0] - top[..., 1] > band) if C1 > 2 else torch.ones(Fr, Q, dtype=torch.bool)
    assert decided.double().mean() > 0.9 and torch.equal(labels[decided], want.max(-1)[1][decided])
    if Q > 1:
        assert int(labels[0, 1]) == 0


# ------------------------------------------------------------------------------------------------
# b. packed masks, c. intersections
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 31, 32, 33, 851, 2048])
def test_pack_kernel(P):
    nat, dev, rows = _nat(), gpu_device(), 5
    x = torch.from_numpy(np.random.RandomState(P).standard_normal((rows, P)).astype(np.float32))
    x[0, ::3] = 0.0                                          # zero is not above zero
    x[1] = -1.0
    x[2] = 1.0
    words = (P + 31) // 32
    bits, area = _ints(dev, rows * words), _ints(dev, rows)
    xd = x.to(dev)
    nat.check(nat.lib.sf_op_vis_pack_masks(xd.data_ptr(), rows, P, bits.data_ptr(), area.data_ptr(), _stream()))
    got = _read_ints(bits, rows * words).view(rows, words).numpy().view(np.uint32)
    assert np.array_equal(got, VO.pack_bits((x > 0).numpy())), "bits differ from x > 0 (tail bits included)"
    assert _read_ints(area, rows).tolist() == (x > 0).sum(-1).tolist()


@pytest.mark.parametrize("Q", [1, 2, 17, 100])
def test_inter_kernel(Q):
    nat, dev, Fr, P = _nat(), gpu_device(), 2, 851
    m = np.random.RandomState(Q).random_sample((Fr, Q, P)) < 0.4
    m[0, 0] = True
    bits = torch.from_numpy(VO.pack_bits(m).view(np.int32)).to(dev)
    inter = _ints(dev, Fr * Q * Q)
    nat.check(nat.lib.sf_op_vis_mask_iou(bits.data_ptr(), Fr, Q, P, inter.data_ptr(), _stream()))
    b = torch.from_numpy(m).long()
    assert torch.equal(_read_ints(inter, Fr * Q * Q).view(Fr, Q, Q).long(), b @ b.transpose(1, 2))


# ------------------------------------------------------------------------------------------------
# d. post-processing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VO.POST_CASES))
def test_postprocess_kernel(name):
    nat, dev, c = _nat(), gpu_device(), VO.POST_CASES[name]
    det, index = VO.make_post_inputs(name)
    (R, h, w), (K, Fr), (H, W) = det.shape, index.shape, c["out"]
    dd, idx = det.to(dev), index.to(dev)
    n = K * Fr * H * W
    ws = torch.empty(nat.lib.sf_op_vis_postprocess_workspace_bytes(K, Fr, H, W), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        mbuf = torch.full((n + 64,), 0x5a, dtype=torch.uint8, device=dev)
        lbuf, logits = guarded(dev, K, Fr, H, W)
        nbuf, num = guarded(dev, K)
        den = torch.full((K + 8,), -7, dtype=torch.int64, device=dev)
        nat.check(nat.lib.sf_op_vis_postprocess(dd.data_ptr(), R, h, w, idx.data_ptr(), K, Fr, c["padded"][0], c["padded"][1], c["crop"][0], c["crop"][1], H, W,
                                                mbuf.data_ptr(), logits.data_ptr(), num.data_ptr(), den.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        mh, dh = mbuf.cpu(), den.cpu()
        assert (mh[n:] == 0x5a).all() and (dh[K:] == -7).all(), "guard bytes were written"
        assert int(mh[:n].max()) <= 1, "a bool byte is 0 or 1"
        runs.append((mh[:n].view(K, Fr, H, W).bool(), read_guarded(lbuf, logits), read_guarded(nbuf, num), dh[:K]))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    bits, got, num, den = runs[0]
    want, want_num, _ = VO.post_reference(det, index, c)
    floor, floor_num, _ = VO.post_reference(det, index, c, dtype=torch.float32)
    check_against_floor(f"{name} logits", got, floor, want)
    band = MARGIN * max(maxabs(floor, want), EPS32 * float(want.abs().max()))
    present = (index >= 0)[:, :, None, None].expand_as(want)
    decided = (want.abs() > band) | ~present
    share = float((~decided)[present].double().mean())
    print(f"  {name}: band {band:.3e}, undecided share {share:.5f}")
    assert share <= CAP
    assert torch.equal(bits[decided], (want > 0)[decided]), "a decided bit differs"
    assert torch.equal(bits, got > 0), "the bits are not the kernel's own logits above zero"
    assert not bits[~present].any() and not got[~present].any(), "an absent entry is not zero"
    assert den.tolist() == bits.flatten(1).sum(1).tolist(), "the denominator is not the popcount of the kernel's own bits"
    check_against_floor(f"{name} numerator", num, floor_num, want_num)


def test_capacity_refusals_come_before_any_launch():
    """What the kernels cannot hold is refused by name with SF_ERR_CAPACITY: a mask row above the 64 KB of LDS of the intersection kernel,
    more planes than one grid, an output tile that reaches more source pixels than the LDS holds."""
    nat, dev = _nat(), gpu_device()
    buf = torch.zeros(1024, dtype=torch.float32, device=dev)
    p = buf.data_ptr()
    assert nat.lib.sf_op_vis_mask_iou(p, 1, 1, 32 * 16384 + 1, p, _stream()) == nat.SF_ERR_CAPACITY and b"LDS" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_vis_postprocess(p, 1, 4, 4, p, 256, 256, 4, 4, 4, 4, 4, 4, p, None, None, None, None, 0, _stream()) == nat.SF_ERR_CAPACITY
    assert b"planes" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_vis_postprocess(p, 1, 64, 300, p, 1, 1, 64, 300, 64, 300, 16, 256, p, None, None, None, None, 0, _stream()) == nat.SF_ERR_CAPACITY
    assert b"LDS" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_vis_postprocess(p, 1, 4, 4, p, 1, 1, 4, 4, 5, 4, 4, 4, p, None, None, None, None, 0, _stream()) == nat.SF_ERR_INVALID
    torch.cuda.synchronize()
    assert not buf.any()


def test_dense_gather_is_exact():
    import streamformer_amd.vis as vis
    dev = gpu_device()
    det, index = VO.make_post_inputs("down")
    hw = tuple(det.shape[1:])
    got = vis.resample_masks(det.to(dev), index.to(dev), hw, hw, hw, masks=False, logits=True, sums=False)["logits"].cpu()
    want = det[index.long().clamp(min=0)]
    want[index < 0] = 0
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------
# the tracker and the post-processing against F25
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return VO.load_golden()


@functools.lru_cache(maxsize=None)
def _det():
    return VO.make_scenario()


@pytest.mark.parametrize("case", list(VO.CASES))
def test_tracker_against_f25(case, monkeypatch):
    import streamformer_amd as sa
    import streamformer_amd.vis as vis
    g, dev, kw = _golden(), gpu_device(), VO.tracker_kwargs(case)
    det = {k: v.to(dev) for k, v in _det().items()}
    copies = []
    real = vis._device_to_host
    monkeypatch.setattr(vis, "_device_to_host", lambda t: (copies.append(t.numel()), real(t))[1])
    trk = sa.SimpleTracker(**kw)
    out = trk.inference(det, hybrid_embed=None)
    assert len(copies) == 1, f"{len(copies)} device-to-host copies inside inference"
    VO.check_trace(trk.trace, case, g, _det(), check_against_floor)
    assert list(trk.video) == g[f"{case}.instances"].tolist()
    index = torch.from_numpy(g[f"{case}.index"])
    assert torch.equal(out["mask_index"].cpu(), index) and out["mask_index"].dtype == torch.int32
    want = torch.from_numpy(g[f"{case}.logits"])
    floor = VO.track(_det(), kw, dtype=torch.float32)["logits"]
    check_against_floor(f"{case} final logits", out["pred_logits"][0], floor, want)
    K = index.shape[0]
    assert out["pred_logits"].shape == (1, K, VO.CLASSES + 1) and out["pred_masks"].shape == (1, K, VO.FRAMES, VO.MASK_H, VO.MASK_W)
    assert torch.equal(out["pred_masks"][0].cpu(), VO.dense_masks(_det(), index, dtype=torch.float32)), "the dense masks are not the gathered rows"
    # frames one at a time: step x F + finish is inference
    online = sa.SimpleTracker(**kw)
    for f in range(VO.FRAMES):
        online.step({k: v[f] for k, v in det.items()})
    fin = online.finish(dense_masks=True)
    assert len(copies) == 1 + VO.FRAMES
    for k in ("pred_logits", "mask_index", "pred_masks"):
        assert torch.equal(fin[k], out[k]), k
    t64 = VO.track({k: v.double() for k, v in _det().items()}, kw)
    m64 = VO.dense_masks({k: v.double() for k, v in _det().items()}, t64["index"])
    m32 = VO.dense_masks(_det(), t64["index"], dtype=torch.float32)
    for gname, geo in VO.GEOMETRIES.items():
        name = f"{case}.{gname}"
        args = ((VO.FRAMES, 3) + tuple(geo["padded"]), geo["crop"], geo["out"][0], geo["out"][1], VO.CLASSES, VO.NUM_TOPK)
        video = sa.postprocess_video_masks(out["pred_logits"], (out["det_masks"], out["mask_index"]), *args, to_store="cpu", test_interpolate_chunk_size=5,
                                           test_instance_chunk_size=5)
        dense = sa.postprocess_video_masks(out["pred_logits"], out["pred_masks"], *args)
        assert video["image_size"] == tuple(geo["out"]) and video["pred_labels"] == g[f"{name}.labels"].tolist()
        assert isinstance(video["pred_scores"], list) and len(video["pred_masks"]) == VO.NUM_TOPK
        masks = torch.stack(video["pred_masks"])
        assert masks.dtype == torch.bool and masks.device.type == "cpu" and masks.shape == (VO.NUM_TOPK, VO.FRAMES) + tuple(geo["out"])
        assert dense["pred_scores"] == video["pred_scores"] and torch.equal(torch.stack(dense["pred_masks"]), masks), "dense and indexed inputs differ"
        assert np.array_equal(VO.pack_bits(masks.flatten(1).numpy()), g[f"{name}.masks"]), "output masks differ from F25"
        floor_scores = VO.inference_video(floor, m32, geo)["scores"]
        assert maxabs(VO.inference_video(t64["logits"], m64, geo)["scores"], g[f"{name}.scores"]) <= 1e-12
        check_against_floor(f"{name} output scores", torch.tensor(video["pred_scores"]), floor_scores, torch.from_numpy(g[f"{name}.scores"]))


# ------------------------------------------------------------------------------------------------
# the segmenter: padding, windows, concatenation
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _modules():
    import streamformer_amd as sa
    from tests import mask_decoder_oracle as DO
    from tests import pixel_decoder_oracle as PO
    from tests import vit_adapter_oracle as AO
    dev = gpu_device()
    ac = AO.CASES["sq"]
    backbone = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(AO.config(ac), **AO.adapter_kwargs(ac))
    backbone.load_state_dict(AO.make_weights(ac), strict=True)
    pc = dict(PO.CASES["m2f"], channels=(ac["hidden"],) * 4)
    pix = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, pc["channels"], PO.STRIDES)}, **PO.decoder_kwargs(pc))
    pix.load_state_dict(PO.make_weights(pc), strict=True)
    dc = dict(DO.CASES["cl"], in_channels=pc["conv_dim"], mask_dim=pc["mask_dim"])
    dec = getattr(sa, dc["cls"])(dc["in_channels"], **DO.decoder_kwargs(dc))
    dec.load_state_dict(DO.make_weights(dc), strict=True)
    return backbone.to(dev).eval(), pix.to(dev).eval(), dec.to(dev).eval(), dc["classes"]


def test_segmenter_wiring():
    import streamformer_amd as sa
    dev = gpu_device()
    backbone, pix, dec, classes = _modules()
    kw = dict(VO.BASE, num_classes=classes, inference_select_thr=0.0, init_score_thr=0.0)
    mean, std = (0.5, 0.25, 0.0), (1.0, 2.0, 0.5)
    seg = sa.VideoInstanceSegmenter(backbone, pix, dec, sa.SimpleTracker(**kw), num_topk=3, num_clip_frames=2, size_divisibility=32, pixel_mean=mean,
                                    pixel_std=std).to(dev).eval()
    frames = [torch.from_numpy(np.random.RandomState(70 + i).standard_normal((3, 50, 60)).astype(np.float32)) for i in range(3)]
    video = seg([{"image": frames, "height": 75, "width": 91}])
    # by hand: normalise, pad to 64 x 64, windows of 2 + 1 frames, concatenate, track, post-process
    batch = torch.zeros(3, 3, 64, 64, device=dev)
    for i, x in enumerate(frames):
        batch[i, :, :50, :60] = (x.to(dev) - torch.tensor(mean, device=dev).view(3, 1, 1)) / torch.tensor(std, device=dev).view(3, 1, 1)
    parts = []
    for clip in (batch[:2], batch[2:]):
        mf, _, ms = pix.forward_features(backbone(pixel_values=clip[None]))
        parts.append(dec(ms, mf))
    det = {k: torch.cat([p[k] for p in parts]) for k in ("pred_logits", "pred_masks", "pred_embeds", "pred_queries")}
    tracked = sa.SimpleTracker(**kw).inference(det, dense_masks=False)
    assert len(tracked["pred_logits"]) == 1 and tracked["pred_logits"].shape[1] >= 1
    want = sa.postprocess_video_masks(tracked["pred_logits"], (tracked["det_masks"], tracked["mask_index"]), (3, 3, 64, 64), (50, 60), 75, 91, classes, 3,
                                      to_store=dev)
    assert video["image_size"] == (75, 91) and video["pred_scores"] == want["pred_scores"] and video["pred_labels"] == want["pred_labels"]
    assert len(video["pred_masks"]) == len(want["pred_masks"]) >= 1
    for a, b in zip(video["pred_masks"], want["pred_masks"]):
        assert a.shape == (3, 75, 91) and a.dtype == torch.bool and torch.equal(a, b)
    # no detection above the thresholds: the reference's empty dict
    none = sa.VideoInstanceSegmenter(backbone, pix, dec, sa.SimpleTracker(**dict(kw, init_score_thr=2.0)), num_topk=3, num_clip_frames=2, pixel_mean=mean,
                                     pixel_std=std).to(dev).eval()
    assert none([{"image": frames}]) == {"image_size": ((50, 60), (50, 60)), "pred_scores": [], "pred_labels": [], "pred_masks": []}
