"""Image segmentation on the MI355X: the three kernels of csrc/sf_seg.hip alone against fp64 torch, the three inference functions against
fixture F26 (the reference's own functions; tests/seg_oracle.py restates them), and ImageSegmenter's wiring.

The method is tests/test_vis.py's: a float is bound by MARGIN = 4 times the PRECISION FLOOR of what it bounds (the error, against fp64, of
the reference's operator sequence in fp32 torch on the CPU, never less than one fp32 rounding of the result), computed from the inputs and
never from the code under test.  A pixel of the panoptic argmax is compared where it is DECIDED: where the fp64 gap between the best and
the second-best score x sigmoid, and |r| of the winner, both exceed their band of 4 x floor; at most CAP = 1 % of the pixels may be
undecided (tests/test_seg_cpu.py shows the inputs stay under it by the reference alone).  Every kernel runs twice with equal bits, into
guarded buffers.
"""
import functools

import numpy as np
import pytest
import torch

from tests import seg_oracle as SO
from tests import vis_oracle as VO
from tests.helpers import check_against_floor, gpu_device, guarded, read_guarded
from tests.helpers import native as _nat, stream as _stream, guarded_ints as _ints, read_guarded_ints as _read_ints

pytestmark = pytest.mark.gpu
CAP = 0.01


def _geo_args(src, g):
    return (src[0], src[1], g["padded"][0], g["padded"][1], g["crop"][0], g["crop"][1], g["out"][0], g["out"][1])


# ------------------------------------------------------------------------------------------------
# a. the semantic kernel
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _semantic_reference(Q, C, gname, before):
    cls, masks = SO.make_kernel_logits(Q, C, 100 * Q + C), SO.make_kernel_masks(Q, 26 + Q)
    g = VO.GEOMETRIES[gname]
    return cls, masks, SO.semantic(cls, masks, g, before=before), SO.semantic(cls, masks, g, before=before, dtype=torch.float32)


@pytest.mark.parametrize("gname", list(VO.GEOMETRIES))
@pytest.mark.parametrize("C", SO.KERNEL_C)
@pytest.mark.parametrize("Q", SO.KERNEL_Q)
def test_semantic_kernel(Q, C, gname):
    """Q in {1, 5, 100}: the query tail of the MFMA K step and more than one chunk of 32; C in {1, 17, 133}: the class tail of its M
    tile; widths 111 and 290 end inside a 64-pixel tile."""
    nat, dev, g = _nat(), gpu_device(), VO.GEOMETRIES[gname]
    cls, masks, want, floor = _semantic_reference(Q, C, gname, True)
    probs = torch.softmax(cls.double(), -1)[:, :-1].float().contiguous().to(dev)      # the kernel's input: fp32 roundings of the fp64 scores
    md = masks.to(dev)
    H, W = g["out"]
    runs = []
    for _ in range(2):
        buf, out = guarded(dev, C, H, W)
        nat.check(nat.lib.sf_op_seg_semantic(md.data_ptr(), probs.data_ptr(), Q, C, *_geo_args(masks.shape[1:], g), out.data_ptr(), _stream()))
        runs.append(read_guarded(buf, out))
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    check_against_floor(f"semantic Q={Q} C={C} {gname}", runs[0], floor, want)


@pytest.mark.parametrize("gname", list(VO.GEOMETRIES))
@pytest.mark.parametrize("before", [True, False])
def test_semantic_inference_both_orders(before, gname):
    import streamformer_amd as sa
    dev, g = gpu_device(), VO.GEOMETRIES[gname]
    cls, masks, want, floor = _semantic_reference(5, 17, gname, before)
    got = sa.semantic_inference(cls.to(dev), masks.to(dev), g, postprocess_before_inference=before)
    assert got.shape == want.shape and got.dtype == torch.float32
    check_against_floor(f"semantic_inference before={before} {gname}", got, floor, want)
    other = SO.semantic(cls, masks, g, before=not before)
    assert float((got.cpu().double() - other).abs().max()) > 1e-3, "the other order would pass too"


# ------------------------------------------------------------------------------------------------
# b. the panoptic argmax, c. relabel
# ------------------------------------------------------------------------------------------------
def _run_argmax(masks, scores, labels, g, threshold, num_classes=SO.CLASSES):
    nat, dev = _nat(), gpu_device()
    Q, (H, W) = masks.shape[0], g["out"]
    md, sd, ld = masks.to(dev), scores.to(dev), labels.to(dev)
    runs = []
    for _ in range(2):
        code, counts = _ints(dev, H * W), _ints(dev, 3 * Q)
        nat.check(nat.lib.sf_op_seg_panoptic_argmax(md.data_ptr(), sd.data_ptr(), ld.data_ptr(), Q, num_classes, threshold, *_geo_args(masks.shape[1:], g),
                                                    code.data_ptr(), counts.data_ptr(), _stream()))
        runs.append((_read_ints(code, H * W).view(H, W), _read_ints(counts, 3 * Q).view(Q, 3)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    return runs[0]


def _counts_of(code, Q):
    """won and both, recomputed from a code map."""
    c = code.flatten().long()
    won = torch.bincount(c[c >= 0] >> 1, minlength=Q)
    both = torch.bincount(c[(c >= 0) & (c & 1 == 1)] >> 1, minlength=Q)
    return won, both


@pytest.mark.parametrize("gname", list(VO.GEOMETRIES))
@pytest.mark.parametrize("Q", SO.PAN_Q)
def test_panoptic_argmax_kernel(Q, gname):
    g = VO.GEOMETRIES[gname]
    masks, scores, labels = SO.make_panoptic_inputs(Q)
    code, counts = _run_argmax(masks, scores, labels, g, SO.PAN_THRESHOLD)
    p64, p32 = SO.panoptic_alone(Q, g), SO.panoptic_alone(Q, g, dtype=torch.float32)
    und = SO.undecided(p64, *SO.bands(p64, p32))
    n_und = int(und.sum())
    print(f"  Q = {Q} {gname}: bands {SO.bands(p64, p32)}, undecided share {n_und / und.numel():.5f}")
    assert n_und <= CAP * und.numel()
    winner = p64["winner"]
    want = 2 * winner + (p64["r"].gather(0, winner.clamp(min=0)[None])[0] >= 0).long()
    assert int(winner.min()) >= 0 and torch.equal(code.long()[~und], want[~und]), "a decided pixel differs"
    won, both = _counts_of(code, Q)
    assert torch.equal(counts[:, 0].long(), won) and torch.equal(counts[:, 2].long(), both), "the counts are not those of the kernel's own code map"
    assert int((counts.long() - torch.from_numpy(p64["counts"])).abs().max()) <= n_und, "counts differ from the oracle's by more than the undecided pixels"
    kept = torch.isfinite(p64["prob"][:, 0, 0])
    assert not counts[~kept].any(), "a query that is not kept has counts"


def test_panoptic_argmax_nothing_kept_and_ties():
    g = VO.GEOMETRIES["down"]
    masks, scores, labels = SO.make_panoptic_inputs(7)
    code, counts = _run_argmax(masks, scores, labels, g, 0.99)
    assert (code == -1).all() and not counts.any()
    code, counts = _run_argmax(masks, scores, torch.full_like(labels, SO.CLASSES), g, 0.0)
    assert (code == -1).all() and not counts.any(), "no-object queries were kept"
    # two identical queries: the lower index wins every pixel
    twice = masks[1:2].repeat(2, 1, 1)
    code, counts = _run_argmax(twice, torch.tensor([0.75, 0.75]), torch.tensor([1, 2], dtype=torch.int32), g, 0.5)
    assert (code >> 1 == 0).all() and counts[1, 0] == 0 and counts[1, 2] == 0 and counts[1, 1] == counts[0, 1] == counts[0, 2]


def test_relabel_kernel():
    import streamformer_amd.segmentation as seg
    nat, dev, Q, H, W = _nat(), gpu_device(), 9, 37, 131
    rs = np.random.RandomState(3)
    code = torch.from_numpy(rs.randint(-1, 2 * Q, size=(H, W)).astype(np.int32))
    table = torch.tensor([3, 0, 1, 1, 0, 7, 2, 0, 5], dtype=torch.int32)
    want = torch.where((code >= 0) & (code & 1 == 1), table[(code >> 1).clamp(min=0).long()], torch.zeros_like(code))
    cd, td = code.to(dev), table.to(dev)
    out = _ints(dev, H * W)
    nat.check(nat.lib.sf_op_seg_panoptic_relabel(cd.data_ptr(), td.data_ptr(), Q, H * W, out.data_ptr(), _stream()))
    assert torch.equal(_read_ints(out, H * W).view(H, W), want) and torch.equal(cd.cpu(), code), "out of place"
    buf = _ints(dev, H * W)
    buf[:H * W] = cd.flatten()
    nat.check(nat.lib.sf_op_seg_panoptic_relabel(buf.data_ptr(), td.data_ptr(), Q, H * W, buf.data_ptr(), _stream()))
    assert torch.equal(_read_ints(buf, H * W).view(H, W), want), "in place"
    assert torch.equal(seg.panoptic_relabel(cd, td).cpu(), want)


def test_refusals_come_before_any_launch():
    """What the kernels cannot hold is refused by name with SF_ERR_CAPACITY: more than 512 queries, more than 256 classes, an output tile
    whose source boxes exceed the LDS (a strong downscale).  The buffers stay as they were."""
    nat, dev = _nat(), gpu_device()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _stream()
    small = (4, 4, 4, 4, 4, 4, 4, 4)
    assert nat.lib.sf_op_seg_semantic(p, p, 513, 4, *small, p, s) == nat.SF_ERR_CAPACITY and b"queries" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_seg_semantic(p, p, 4, 257, *small, p, s) == nat.SF_ERR_CAPACITY and b"classes" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_seg_panoptic_argmax(p, p, p, 513, 4, 0.5, *small, p, p, s) == nat.SF_ERR_CAPACITY and b"queries" in nat.lib.sf_last_error()
    shrink = (64, 4096, 64, 4096, 64, 4096, 2, 64)      # one 64-pixel tile of a row reaches 32 x 4096 source pixels
    assert nat.lib.sf_op_seg_semantic(p, p, 1, 1, *shrink, p, s) == nat.SF_ERR_CAPACITY and b"LDS" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_seg_panoptic_argmax(p, p, p, 1, 4, 0.5, *shrink, p, p, s) == nat.SF_ERR_CAPACITY and b"LDS" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_seg_semantic(p, p, 1, 1, 4, 4, 4, 4, 5, 4, 4, 4, p, s) == nat.SF_ERR_INVALID
    torch.cuda.synchronize()
    assert not buf.any()


# ------------------------------------------------------------------------------------------------
# the three functions against F26
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return SO.load_golden()


@pytest.mark.parametrize("gname", list(SO.GEOMETRIES))
def test_functions_against_f26(gname, monkeypatch):
    import streamformer_amd as sa
    import streamformer_amd.segmentation as seg
    gold, dev, g = _golden(), gpu_device(), SO.GEOMETRIES[gname]
    cls, masks = SO.make_scenario()
    cd, md = cls.to(dev), masks.to(dev)
    copies = []
    real = seg._device_to_host
    monkeypatch.setattr(seg, "_device_to_host", lambda t: (copies.append(t.numel()), real(t))[1])
    for case, kw in SO.CASES.items():
        before = len(copies)
        pan, info = sa.panoptic_inference(cd, md, g, **kw)
        assert len(copies) == before + 1 and copies[-1] == 5 * SO.QUERIES, "one device-to-host copy: scores, labels, counts"
        assert pan.dtype == torch.int32 and pan.shape == tuple(g["out"]) and pan.device.type == "cuda"
        assert np.array_equal(SO.info_array(info), gold[f"{gname}.{case}.info"]), case
        p64, p32 = SO.panoptic(cls, masks, g, kw), SO.panoptic(cls, masks, g, kw, dtype=torch.float32)
        und = SO.undecided(p64, *SO.bands(p64, p32))
        print(f"  {gname}.{case}: undecided share {float(und.double().mean()):.5f}")
        assert float(und.double().mean()) <= CAP
        assert torch.equal(pan.cpu()[~und], torch.from_numpy(gold[f"{gname}.{case}.map"].astype(np.int32))[~und]), case
    for name, things in (("inst", None), ("inst_things", SO.THINGS)):
        r = sa.instance_inference(cd, md, g, num_classes=SO.CLASSES, test_topk_per_image=SO.TOPK, thing_classes=things)
        K = len(gold[f"{gname}.{name}.labels"])
        assert len(r) == K and r.image_size == tuple(g["out"]) and r.pred_classes.tolist() == gold[f"{gname}.{name}.labels"].tolist()
        assert r.pred_masks.dtype == torch.float32 and r.pred_masks.shape == (K,) + tuple(g["out"]) and r.pred_boxes.shape == (K, 4) and not r.pred_boxes.any()
        assert np.array_equal(SO.pack_bits(r.pred_masks.flatten(1).cpu().numpy() > 0.5), gold[f"{gname}.{name}.masks"]), "instance masks differ from F26"
        as_bool = sa.instance_inference(cd, md, g, num_classes=SO.CLASSES, test_topk_per_image=SO.TOPK, thing_classes=things, as_bool=True)
        assert as_bool.pred_masks.dtype == torch.bool and torch.equal(as_bool.pred_masks, r.pred_masks > 0.5) and torch.equal(as_bool.scores, r.scores)
        floor = SO.instance(cls, masks, g, things=things, dtype=torch.float32)["scores"]
        check_against_floor(f"{gname}.{name} scores", r.scores, floor, torch.from_numpy(gold[f"{gname}.{name}.scores"]))
    for before in (True, False):
        got = sa.semantic_inference(cd, md, g, postprocess_before_inference=before)
        want = SO.semantic(cls, masks, g, before=before)
        check_against_floor(f"{gname} semantic before={before}", got, SO.semantic(cls, masks, g, before=before, dtype=torch.float32), want)


# ------------------------------------------------------------------------------------------------
# the segmenter: padding, the three outputs per image
# ------------------------------------------------------------------------------------------------
def test_image_segmenter_wiring():
    import streamformer_amd as sa
    from tests.test_vis import _modules
    dev = gpu_device()
    backbone, pix, dec, classes = _modules()
    mean, std = (0.5, 0.25, 0.0), (1.0, 2.0, 0.5)
    things = tuple(range(classes // 2 + 1))
    kw = dict(object_mask_threshold=0.0, overlap_threshold=0.1, thing_classes=things, size_divisibility=32, pixel_mean=mean, pixel_std=std, semantic_on=True,
              panoptic_on=True, instance_on=True, test_topk_per_image=3)
    images = [torch.from_numpy(np.random.RandomState(80 + i).standard_normal((3,) + hw).astype(np.float32)) for i, hw in enumerate([(50, 60), (40, 64)])]
    inputs = [{"image": images[0], "height": 75, "width": 91}, {"image": images[1], "height": 33, "width": 52}]
    # by hand: normalise, pad both to 64 x 64, one batch of two single-frame clips
    batch = torch.zeros(2, 3, 64, 64, device=dev)
    for i, x in enumerate(images):
        batch[i, :, :x.shape[1], :x.shape[2]] = (x.to(dev) - torch.tensor(mean, device=dev).view(3, 1, 1)) / torch.tensor(std, device=dev).view(3, 1, 1)
    mf, _, ms = pix.forward_features(backbone(pixel_values=batch[:, None]))
    det = dec(ms, mf)
    Q = det["pred_logits"].shape[1]
    for before in (True, False):
        seg = sa.ImageSegmenter(backbone, pix, dec, num_queries=Q, sem_seg_postprocess_before_inference=before, **kw).to(dev).eval()
        results = seg(inputs)
        assert len(results) == 2
        for i, (r, inp) in enumerate(zip(results, inputs)):
            out, size = (inp["height"], inp["width"]), tuple(images[i].shape[1:])
            full = dict(padded=(64, 64), crop=size, out=out)
            geo = full if before else dict(padded=(64, 64), crop=(64, 64), out=(64, 64))
            shape = out if before else (64, 64)
            cls, masks = det["pred_logits"][i], det["pred_masks"][i]
            assert set(r) == {"sem_seg", "panoptic_seg", "instances"}
            assert r["sem_seg"].shape == (classes,) + out
            assert torch.equal(r["sem_seg"], sa.semantic_inference(cls, masks, full, postprocess_before_inference=before))
            pan, info = sa.panoptic_inference(cls, masks, geo, num_classes=classes, object_mask_threshold=0.0, overlap_threshold=0.1, thing_classes=things)
            assert r["panoptic_seg"][0].shape == shape and torch.equal(r["panoptic_seg"][0], pan) and r["panoptic_seg"][1] == info
            inst = sa.instance_inference(cls, masks, geo, num_classes=classes, test_topk_per_image=3, thing_classes=things)
            got = r["instances"]
            assert got.image_size == shape and torch.equal(got.pred_masks, inst.pred_masks) and torch.equal(got.scores, inst.scores)
            assert torch.equal(got.pred_classes, inst.pred_classes) and got.pred_masks.shape[1:] == shape
    with pytest.raises(ValueError, match="num_queries"):
        sa.ImageSegmenter(backbone, pix, dec, num_queries=Q + 1, **kw).to(dev).eval()(inputs)
