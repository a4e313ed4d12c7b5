"""CPU: the image-segmentation oracle against fixture F26 (the reference's own semantic, panoptic and instance inference), its decision
margins, the host rule of ``panoptic_inference`` and ``ImageSegmenter``'s refusals, without a GPU.

The oracle (tests/seg_oracle.py, fp64) must reproduce F26 exactly on every discrete output and to 1e-12 on every float; every decision
has a relative margin of at least 1e-3 and every overlap decision survives moving each area by the number of undecided pixels; the
oracle in fp32 takes every decision the same way.  The inputs of the argmax kernel's own test (tests/test_seg.py) are checked here for
what its bound needs: the share of pixels inside the bands stays under the 1 % cap by the fp32 reference alone.
"""
import numpy as np
import pytest
import torch

from tests import seg_oracle as SO
from tests import vis_oracle as VO
from tests.helpers import maxabs

CAP = 0.01
STRIDE = {"down": 2, "up": 3}


@pytest.fixture(scope="module")
def golden():
    return SO.load_golden()


@pytest.fixture(scope="module")
def scenario(golden):
    cls, masks = SO.make_scenario()
    assert torch.equal(cls, torch.from_numpy(golden["mask_cls"].astype(np.float32))), "the stored inputs are not the seeded scenario"
    assert torch.equal(masks, torch.from_numpy(golden["mask_pred"].astype(np.float32)))
    return cls, masks


@pytest.mark.parametrize("gname", list(SO.GEOMETRIES))
def test_oracle_reproduces_f26(gname, golden, scenario):
    cls, masks = scenario
    g = SO.GEOMETRIES[gname]
    smallest = np.inf
    for name, before in (("before", True), ("after", False)):
        sem = SO.semantic(cls, masks, g, before=before)
        assert sem.shape == (SO.CLASSES,) + tuple(g["out"])
        assert maxabs(sem[:, ::STRIDE[gname], ::STRIDE[gname]], golden[f"{gname}.sem_{name}"]) <= 1e-12, name
    assert maxabs(SO.semantic(cls, masks, g, before=True), SO.semantic(cls, masks, g, before=False)) > 1e-3, "the two orders must differ"
    for case, kw in SO.CASES.items():
        p64, p32 = SO.panoptic(cls, masks, g, kw), SO.panoptic(cls, masks, g, kw, dtype=torch.float32)
        for p in (p64, p32):
            assert np.array_equal(p["map"].numpy(), golden[f"{gname}.{case}.map"].astype(np.int32)), case
            assert np.array_equal(SO.info_array(p["segments_info"]), golden[f"{gname}.{case}.info"]), case
            assert p["segment_of_query"] == golden[f"{gname}.{case}.segment_of_query"].tolist()
            assert np.array_equal(p["counts"], golden[f"{gname}.{case}.counts"]), case
        slack = int(SO.undecided(p64, *SO.bands(p64, p32)).sum())
        assert slack <= CAP * p64["map"].numel() and SO.overlap_decisions_hold(p64, kw, slack), (case, slack)
        smallest = min([smallest] + [m for _, m in p64["margins"]])
    for name, things in (("inst", None), ("inst_things", SO.THINGS)):
        i64, i32 = SO.instance(cls, masks, g, things=things), SO.instance(cls, masks, g, things=things, dtype=torch.float32)
        for i in (i64, i32):
            assert i["labels"].tolist() == golden[f"{gname}.{name}.labels"].tolist() and i["rows"].tolist() == golden[f"{gname}.{name}.rows"].tolist()
        assert maxabs(i64["scores"], golden[f"{gname}.{name}.scores"]) <= 1e-12
        assert np.array_equal(SO.pack_bits(i64["masks"].flatten(1).numpy()), golden[f"{gname}.{name}.masks"])
        smallest = min([smallest] + [m for _, m in i64["margins"]])
    assert smallest >= SO.MIN_MARGIN


def test_scenario_holds_what_it_plants(golden):
    """Two merged stuff queries, a query under the score threshold, a no-object query, an occluded query under the overlap threshold, a
    kept query that wins nothing, two overlapping things that both survive."""
    for gname in SO.GEOMETRIES:
        seg, counts = golden[f"{gname}.planted.segment_of_query"].tolist(), golden[f"{gname}.planted.counts"]
        assert seg[0] == seg[1] == 1 and golden[f"{gname}.planted.info"].tolist()[0] == [1, 0, 3]
        assert seg[2] == 0 and not counts[2].any() and seg[3] == 0 and not counts[3].any()
        assert seg[5] == 0 and counts[5][0] > 0 and counts[5][2] > 0 and counts[5][0] / counts[5][1] < 0.5
        assert seg[6] == 0 and counts[6][0] == 0 and counts[6][1] > 0
        assert seg[7] > 0 and seg[8] > 0 and seg[7] != seg[8] and counts[8][0] < counts[8][1]
        assert not golden[f"{gname}.nothing.map"].any() and golden[f"{gname}.nothing.info"].shape == (0, 3)


@pytest.mark.parametrize("gname", list(SO.GEOMETRIES))
def test_host_rule_on_f26_counts(gname, golden, scenario):
    import streamformer_amd as sa
    cls, _ = scenario
    scores, labels = torch.softmax(cls, -1).max(-1)
    for case, kw in SO.CASES.items():
        info, seg = sa.panoptic_segments_host(scores.tolist(), labels.tolist(), golden[f"{gname}.{case}.counts"].tolist(), **kw)
        assert np.array_equal(SO.info_array(info), golden[f"{gname}.{case}.info"]) and seg == golden[f"{gname}.{case}.segment_of_query"].tolist()
        assert all(set(s) == {"id", "isthing", "category_id"} and isinstance(s["isthing"], bool) for s in info)


def test_host_rule_keeps_nothing():
    import streamformer_amd as sa
    info, seg = sa.panoptic_segments_host([0.9, 0.4, 0.7], [5, 1, 2], [[9, 9, 9], [9, 9, 9], [0, 4, 0]], num_classes=5, object_mask_threshold=0.5,
                                          overlap_threshold=0.5, thing_classes=(0, 1, 2))
    assert info == [] and seg == [0, 0, 0]


@pytest.mark.parametrize("gname", list(VO.GEOMETRIES))
@pytest.mark.parametrize("Q", SO.PAN_Q)
def test_argmax_inputs_are_decided_by_the_reference_alone(Q, gname):
    g = VO.GEOMETRIES[gname]
    p64, p32 = SO.panoptic_alone(Q, g), SO.panoptic_alone(Q, g, dtype=torch.float32)
    und = SO.undecided(p64, *SO.bands(p64, p32))
    share = float(und.double().mean())
    print(f"  Q = {Q} {gname}: bands {SO.bands(p64, p32)}, undecided share {share:.5f}")
    assert share <= CAP
    assert torch.equal(p32["winner"][~und], p64["winner"][~und])
    if Q > 1:
        kept = torch.isfinite(p64["prob"][:, 0, 0])
        assert 1 < int(kept.sum()) < Q, "the inputs must hold kept and dropped queries"


def test_segmenter_refusals():
    import streamformer_amd as sa
    parts = (torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity())
    with pytest.raises(AssertionError):
        sa.ImageSegmenter(*parts, num_queries=4, semantic_on=False, instance_on=True, sem_seg_postprocess_before_inference=False)
    seg = sa.ImageSegmenter(*parts, num_queries=4, semantic_on=True, sem_seg_postprocess_before_inference=False)
    assert seg.training
    with pytest.raises(NotImplementedError, match="criterion.*matcher"):
        seg([{"image": torch.zeros(3, 8, 8)}])
