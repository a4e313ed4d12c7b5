"""CPU: the video-instance-segmentation oracle against fixture F25 (the reference's own tracker and inference_video), the decision margins,
and SimpleTracker's host loop, its refusals and the empty returns, without a GPU.

The oracle (tests/vis_oracle.py, fp64) must reproduce F25 exactly on every discrete output and to 1e-12 on every float, and F25's
smallest decision margin must be at least 1e-3 relative.  The library's host loop (``SimpleTracker.step_host``, fp32 torch CPU ops) is fed
the oracle's scores, intersections and areas in fp32 and must reproduce F25's selections, ids, instance table and index table exactly
and its final logits within MARGIN x the fp32 floor.  The post-processing cases of tests/test_vis.py are checked here for what their
bound needs: the share of output pixels whose fp64 logit lies inside the band of 4 x floor stays under the 1 % cap by the reference
alone.
"""
import functools

import numpy as np
import pytest
import torch

from tests import vis_oracle as VO
from tests.helpers import EPS32, MARGIN, check_against_floor, maxabs

CAP = 0.01


@functools.lru_cache(maxsize=None)
def _golden():
    return VO.load_golden()


@functools.lru_cache(maxsize=None)
def _det():
    g = _golden()
    det = {k: torch.from_numpy(g[k].astype(np.float32)) for k in ("pred_logits", "pred_masks", "pred_embeds", "pred_queries")}
    made = VO.make_scenario()
    assert all(torch.equal(det[k], made[k]) for k in det), "the stored inputs are not the seeded scenario"
    return det


@functools.lru_cache(maxsize=None)
def _tracked(case):
    return VO.track({k: v.double() for k, v in _det().items()}, VO.tracker_kwargs(case))


@pytest.mark.parametrize("case", list(VO.CASES))
def test_oracle_reproduces_f25_tracker(case):
    g, t = _golden(), _tracked(case)
    for k in ("selected", "kept", "ids"):
        assert VO.unragged(g[f"{case}.{k}"]) == t[k], k
    assert g[f"{case}.instances"].tolist() == t["instances"]
    assert np.array_equal(g[f"{case}.index"], t["index"])
    assert maxabs(t["logits"], g[f"{case}.logits"]) <= 1e-12
    assert VO.unragged(g[f"{case}.bank_ids"]) == t["bank_ids"]
    for f, e in enumerate(t["bank_embeds"]):
        stored = g[f"{case}.bank_embeds"][f]
        n = 0 if e is None else e.shape[0]
        assert not stored[n:].any() and (e is None or maxabs(e, stored[:n]) <= 1e-12), f


def test_no_alternative_is_indistinguishable_from_the_default():
    """What the tests compare differs between the default and every alternative, and between the embed types: a tracker that ignored
    ``match_type``, ``match_metric``, ``embed_type`` or ``temporal_score_type`` cannot pass."""
    g, d = _golden(), _tracked("default")
    assert not np.array_equal(g["hungarian.ids"], g["default.ids"]) and not np.array_equal(g["hungarian.index"], g["default.index"])
    X, Y = 5 * VO.QUERIES + 9, 5 * VO.QUERIES + 10
    assert g["default.index"][1, 5] == X and g["hungarian.index"][1, 5] == Y and g["hungarian.index"][2, 5] == X
    embeds = {c: g[f"{c}.bank_embeds"] for c in ("default", "last", "weighted", "momentum")}
    names = list(embeds)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert embeds[a].shape != embeds[b].shape or np.abs(embeds[a] - embeds[b]).max() > 1e-3, (a, b)
    cos = _tracked("cosine")
    assert max(float((a - b).abs().max()) for a, b in zip(cos["match"], d["match"]) if a is not None) > 1e-3
    assert np.abs(g["max.logits"] - g["default.logits"]).max() > 1e-3
    assert any(g[f"max.{n}.labels"].tolist() != g[f"default.{n}.labels"].tolist() for n in VO.GEOMETRIES)


def test_scenario_fires_every_rule():
    g = _golden()
    sel, kept, ids = (VO.unragged(g[f"default.{k}"]) for k in ("selected", "kept", "ids"))
    index = g["default.index"]
    assert all(6 in s and 6 not in k for s, k in zip(sel, kept)), "the duplicate of A is selected and removed by NMS in every frame"
    assert all(5 in k for k in kept) and index.shape == (4, VO.FRAMES), "the faint detection is kept but never tracked; D is deleted"
    assert index[1, 4] == -1 and index[1, 5] == 5 * VO.QUERIES + 9 and (index[1, 6:] >= 0).all(), "B is away for two frames (X takes its tracklet in frame 5) and returns under its id"
    assert (index[2, 3:] == -1).all() and (index[2, :3] >= 0).all(), "C stops after frame 2"
    assert sorted(i for f in ids for i in f if i > 3) == [4, 5, 5] and g["default.instances"].tolist() == [0, 1, 2, 3], "Y (one frame) and D (two) were deleted as noise"


def test_oracle_reproduces_f25_post_processing_and_margins():
    g = _golden()
    smallest = min(m for c in VO.CASES for _, m in _tracked(c)["margins"])
    for case, gname in ((c, n) for c in VO.CASES for n in VO.GEOMETRIES):
        t, geo, name = _tracked(case), VO.GEOMETRIES[gname], f"{case}.{gname}"
        masks = VO.dense_masks({k: v.double() for k, v in _det().items()}, t["index"])
        v = VO.inference_video(t["logits"], masks, geo)
        assert v["labels"].tolist() == g[f"{name}.labels"].tolist() and v["rows"].tolist() == g[f"{name}.rows"].tolist()
        assert maxabs(v["scores"], g[f"{name}.scores"]) <= 1e-12 and maxabs(v["numerator"], g[f"{name}.numerator"]) <= 1e-12 * float(v["numerator"].max())
        assert v["denominator"].long().tolist() == g[f"{name}.denominator"].tolist()
        assert np.array_equal(VO.pack_bits(v["masks"].flatten(1).numpy()), g[f"{name}.masks"])
        smallest = min([smallest] + [m for _, m in v["margins"]])
    print(f"  smallest decision margin {smallest:.3e}")
    assert smallest >= VO.MIN_MARGIN


def _host_inputs(det, f):
    fr = VO.front(det)
    return (fr["max_scores"][f].float(), det["pred_logits"][f], fr["inter"][f].to(torch.int32), fr["area"][f].to(torch.int32), det["pred_embeds"][f],
            det["pred_queries"][f])


def _run_host(trk, det):
    trk.reset()
    for f in range(det["pred_logits"].shape[0]):
        trk.step_host(*_host_inputs(det, f))
    return trk.finish()


@pytest.mark.parametrize("case", list(VO.CASES))
def test_host_loop_reproduces_f25(case):
    import streamformer_amd as sa
    g, det, kw = _golden(), _det(), VO.tracker_kwargs(case)
    trk = sa.SimpleTracker(**kw)
    out = _run_host(trk, det)
    VO.check_trace(trk.trace, case, g, det, check_against_floor)
    assert list(trk.video) == g[f"{case}.instances"].tolist()
    assert out["mask_index"].dtype == torch.int32 and np.array_equal(out["mask_index"].numpy(), g[f"{case}.index"])
    assert out["pred_logits"].shape == (1,) + g[f"{case}.logits"].shape
    floor = VO.track(det, kw, dtype=torch.float32)["logits"]
    check_against_floor(f"{case} final logits", out["pred_logits"][0], floor, torch.from_numpy(g[f"{case}.logits"]))
    again = _run_host(trk, det)                              # reset() forgets everything: a second clip gives the same bits
    assert torch.equal(again["pred_logits"], out["pred_logits"]) and torch.equal(again["mask_index"], out["mask_index"])


def test_constructor_defaults_and_refusals():
    import inspect
    import streamformer_amd as sa
    p = inspect.signature(sa.SimpleTracker.__init__).parameters
    want = dict(match_metric="bisoftmax", match_score_thr=0.2, temporal_score_type="mean", match_type="greedy", inference_select_thr=0.01,
                init_score_thr=0.01, mask_nms_thr=0.6, frame_weight=True, noise_frame_num=8, noise_frame_ratio=0.4, suppress_frame_num=3,
                none_frame_num=2, num_dead_frames=20, embed_type="similarity_guided", maximum_cache=10)
    assert {k: p[k].default for k in want} == want and all(p[k].kind is p[k].KEYWORD_ONLY for k in want)
    with pytest.raises(NotImplementedError, match="hybrid"):
        sa.SimpleTracker(num_classes=5, temporal_score_type="hybrid")
    for field, value in (("match_metric", "euclid"), ("match_type", "auction"), ("embed_type", "mean")):
        with pytest.raises(NotImplementedError, match=field):
            sa.SimpleTracker(num_classes=5, **{field: value})
    det = _det()
    with pytest.raises(RuntimeError, match="MI355X"):
        sa.SimpleTracker(num_classes=5).inference(det)
    with pytest.raises(RuntimeError, match="MI355X"):
        sa.postprocess_video_masks(det["pred_logits"][:1], det["pred_masks"][:1, :, None], (1, 3, 92, 148), (90, 145), 67, 111, 5, 4)
    seg = sa.VideoInstanceSegmenter(torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity(), sa.SimpleTracker(num_classes=5), num_topk=4)
    assert not list(seg.parameters())
    with pytest.raises(NotImplementedError, match="inference only"):
        seg.train()([{"image": [torch.zeros(3, 8, 8)]}])


def test_hungarian_names_scipy_when_it_is_missing(monkeypatch):
    import builtins
    import streamformer_amd as sa
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError("No module named 'scipy'")
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="scipy"):
        sa.SimpleTracker(num_classes=5, match_type="hungarian")


def test_empty_returns():
    import streamformer_amd as sa
    assert sa.postprocess_video_masks([], None, (1, 3, 92, 148), (90, 145), 67, 111, 5, 4) == {"image_size": (67, 111), "pred_scores": [], "pred_labels": [],
                                                                                              "pred_masks": []}
    trk = sa.SimpleTracker(**dict(VO.tracker_kwargs("default"), init_score_thr=2.0))      # nothing is ever started
    out = _run_host(trk, _det())
    assert out["pred_logits"] == [] and out["mask_index"].shape == (0, VO.FRAMES)
    assert all(len(t["selected"]) >= 1 and t["ids"] == [] for t in trk.trace)


@pytest.mark.parametrize("name", list(VO.POST_CASES))
def test_post_cases_stay_under_the_undecided_cap(name):
    c = VO.POST_CASES[name]
    det, index = VO.make_post_inputs(name)
    want, _, _ = VO.post_reference(det, index, c)
    floor, _, _ = VO.post_reference(det, index, c, dtype=torch.float32)
    band = MARGIN * max(maxabs(floor, want), EPS32 * float(want.abs().max()))
    present = (index >= 0)[:, :, None, None].expand_as(want)
    share = float((want[present].abs() <= band).double().mean())
    print(f"  {name}: band {band:.3e}, undecided share {share:.5f}")
    assert share <= CAP
    assert (index < 0).any() == (c["K"] * c["F"] > 1)
