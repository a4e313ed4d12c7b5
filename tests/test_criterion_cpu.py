"""CPU: the criterion oracle (tests/criterion_oracle.py) against fixture F27 = the reference's own SetCriterion / HungarianMatcher in
fp64, the three conditions on the planted scenario (agreement, assignment margin, undecided points), and the host-side logic of
streamformer_amd/criterion.py that needs no device: draws, pair table, assignment, num_masks, dict keys, refusals."""
import os

import numpy as np
import pytest
import torch

from tests import criterion_oracle as CO
from tests.helpers import load_npz

CASE_NAMES = sorted(CO.CASES)
_RUNS = {}


def oracle(name, dtype):
    if (name, dtype) not in _RUNS:
        _RUNS[name, dtype] = CO.run(CO.CASES[name] if name in CO.CASES else CO.EXTRA[name], dtype)
    return _RUNS[name, dtype]


@pytest.fixture(scope="module")
def f27(golden_dir):
    return load_npz(os.path.join(golden_dir, "f27_criterion.npz"))


def test_scenario_shapes_are_the_planted_ones():
    c = CO.CASES["main"]
    assert (c["L"], c["B"], c["G"], c["Q"], c["C"], c["pred"], c["K"]) == (3, 3, (3, 0, 5), 20, 7, (24, 40), 200)
    assert CO.counts(c) == (200, 600, 150, 50) and (c["w_class"], c["w_mask"], c["w_dice"], c["eos"]) == (2.0, 5.0, 5.0, 0.1)
    layers, targets = CO.scenario(c)
    assert targets[0][1].shape == (3, 96, 160) and targets[2][1][4].sum() == 0 and targets[0][1][0].sum() > 0
    assert max(float(np.abs(m).max()) for _, m in layers) > 25.0                     # softplus and the sigmoid saturate
    assert CO.CASES["q_lt_g"]["Q"] < CO.CASES["q_lt_g"]["G"][0] and len(set(CO.CASES["sizes"]["tgt"])) == 2
    assert CO.counts(CO.CASES["imp0"])[2] == 0 and CO.counts(CO.CASES["imp1"])[3] == 0
    assert CO.counts(CO.CAPACITY) == (12544, 37632, 9408, 3136)
    d = CO.draws(c)[0][0]
    px, py = d[:, 0] * 160 - 0.5, d[:, 1] * 96 - 0.5                                  # points within half a pixel of every border
    assert (px < 0).any() and (px > 159).any() and (py < 0).any() and (py > 95).any()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_agrees_with_the_reference(f27, name):
    """Condition 1: exact on every assignment and chosen index set, 1e-12 on every cost and loss; the draws are the fixture's."""
    case, o = CO.CASES[name], oracle(name, torch.float64)
    assert np.array_equal(CO.checksum(case), f27[f"{name}_checksum"]), "the scenario is not the one the fixture was made from"
    for i, d in enumerate(CO.draws(case)):
        assert np.array_equal(d, f27[f"{name}_draw_{i}"])
    for l in range(case["L"]):
        for b in range(case["B"]):
            want = f27[f"{name}_cost_{l}_{b}"]
            assert o["costs"][l][b].shape == want.shape
            if want.size:
                assert float(np.abs(o["costs"][l][b].numpy() - want).max()) <= 1e-12
            assert np.array_equal(o["indices"][l][b][0].numpy(), f27[f"{name}_src_{l}_{b}"])
            assert np.array_equal(o["indices"][l][b][1].numpy(), f27[f"{name}_tgt_{l}_{b}"])
            assert len(f27[f"{name}_src_{l}_{b}"]) == min(case["Q"], case["G"][b])
        assert np.array_equal(o["chosen"][l].sort(1).values.numpy(), f27[f"{name}_chosen_{l}"])
    assert float(np.abs(o["losses"].numpy() - f27[f"{name}_losses"]).max()) <= 1e-12


@pytest.mark.parametrize("name", CASE_NAMES)
def test_assignment_margin(f27, name):
    """Condition 2: forbidding any one pair of the best assignment costs at least 1e-3 of the largest |cost|; fp32 assigns as fp64."""
    case, o32 = CO.CASES[name], oracle(name, torch.float32)
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert CO.assignment_margin(f27[f"{name}_cost_{l}_{b}"]) >= CO.MARGIN_REL, (l, b)
            assert np.array_equal(o32["indices"][l][b][0].numpy(), f27[f"{name}_src_{l}_{b}"])
            assert np.array_equal(o32["indices"][l][b][1].numpy(), f27[f"{name}_tgt_{l}_{b}"])
    assert float(f27["margin"]) >= CO.MARGIN_REL


@pytest.mark.parametrize("name", CASE_NAMES)
def test_undecided_points(f27, name):
    """Condition 3: at most CAP of a pair's chosen points are undecided; the fp32 oracle's sets differ from the fp64 ones only there."""
    case, o64, o32 = CO.CASES[name], oracle(name, torch.float64), oracle(name, torch.float32)
    ku = CO.counts(case)[2]
    for l in range(case["L"]):
        und = CO.undecided(o64["x_over"][l], o32["x_over"][l], ku)
        if ku:
            assert float(und.sum(1).max()) / ku <= CO.CAP
        assert CO.differs_only_in(o32["chosen"][l], o64["chosen"][l], und)
    assert float(f27["undecided_share"]) <= CO.CAP


@pytest.mark.parametrize("name", sorted(CO.EXTRA))
def test_cases_beside_the_fixture_meet_conditions_2_and_3(name):
    """The cases that are too large for F27 are compared with the oracle alone, under the same margin and undecided-point conditions."""
    case, o64, o32 = CO.EXTRA[name], oracle(name, torch.float64), oracle(name, torch.float32)
    ku = CO.counts(case)[2]
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert CO.assignment_margin(o64["costs"][l][b].numpy()) >= CO.MARGIN_REL, (l, b)
            assert all(torch.equal(a, c) for a, c in zip(o64["indices"][l][b], o32["indices"][l][b]))
        und = CO.undecided(o64["x_over"][l], o32["x_over"][l], ku)
        assert float(und.sum(1).max()) / ku <= CO.CAP
        assert CO.differs_only_in(o32["chosen"][l], o64["chosen"][l], und)


def test_cases_beside_the_fixture_reach_the_other_kernel_paths():
    e = CO.EXTRA
    assert -(-e["capacity"]["K"] // 512) == 25 and all(e[n]["Q"] > 64 and e[n]["K"] > 512 and e[n]["K"] % 64 for n in ("wide2", "wide4", "wide8"))
    assert [-(-max(e[n]["G"]) // 16) for n in ("wide2", "wide4", "wide8")] == [2, 3, 5] and min(e["wide2"]["G"]) <= 16
    big = e["empty_big"]
    assert big["G"][1] == 0 and big["tgt"][1][0] > big["tgt"][0][0] and big["tgt"][1][1] > big["tgt"][0][1]


def test_assignment_margin_sees_a_tie():
    assert CO.assignment_margin(np.asarray([[1.0, 1.0], [1.0, 1.0]])) == 0.0
    assert CO.assignment_margin(np.asarray([[0.0, 5.0], [5.0, 0.0]])) == 2.0
    assert CO.assignment_margin(np.zeros((4, 0))) == float("inf")


# ---------------------------------------------------------------------------------------------------
# host-side logic of the module
# ---------------------------------------------------------------------------------------------------
def test_module_interface_is_the_references():
    import streamformer_amd as sa
    from streamformer_amd import criterion as K
    m = sa.HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=200)
    assert (m.cost_class, m.cost_mask, m.cost_dice, m.num_points, m.rand) == (2.0, 5.0, 5.0, 200, None)
    assert repr(m) == "Matcher HungarianMatcher\n    cost_class: 2.0\n    cost_mask: 5.0\n    cost_dice: 5.0"
    with pytest.raises(AssertionError):
        sa.HungarianMatcher(0, 0, 0)
    c = sa.SetCriterion(7, m, {"loss_ce": 2.0}, 0.1, ["labels", "masks"], 200, 3.0, 0.75)
    assert c.empty_weight.tolist() == [1.0] * 7 + [pytest.approx(0.1)] and "empty_weight" in dict(c.named_buffers())
    assert c.point_counts() == (200, 600, 150)
    assert repr(c) == ("Criterion SetCriterion\n    matcher: Matcher HungarianMatcher\n        cost_class: 2.0\n        cost_mask: 5.0\n"
                       "        cost_dice: 5.0\n    losses: ['labels', 'masks']\n    weight_dict: {'loss_ce': 2.0}\n    num_classes: 7\n"
                       "    eos_coef: 0.1\n    num_points: 200\n    oversample_ratio: 3.0\n    importance_sample_ratio: 0.75")
    assert "matcher: Identity()" in repr(sa.SetCriterion(7, torch.nn.Identity(), {}, 0.1, ["labels"], 8, 3.0, 0.75))      # a foreign matcher
    assert c._trace is None and not hasattr(c, "last_step")
    r = repr(c).split("\n")
    assert r[0] == "Criterion SetCriterion" and r[1].startswith("    matcher: Matcher HungarianMatcher") and r[-1] == "    importance_sample_ratio: 0.75"
    assert K.LOSSES == ("labels", "masks")


def test_refusals_need_no_device():
    import streamformer_amd as sa
    m = sa.HungarianMatcher(num_points=8)
    outputs, targets, _ = CO.tensors(CO.CASES["q_lt_g"], torch.float32)
    for kw, exc, word in ((dict(losses=["labels", "boxes"]), ValueError, "boxes"), (dict(oversample_ratio=0.5), ValueError, "oversample_ratio"),
                          (dict(importance_sample_ratio=1.5), ValueError, "importance_sample_ratio"),
                          (dict(num_points=20000), RuntimeError, "capacity"), (dict(), RuntimeError, "CPU tensors")):
        args = dict(num_classes=7, matcher=m, weight_dict={}, eos_coef=0.1, losses=["labels", "masks"], num_points=8, oversample_ratio=3.0,
                    importance_sample_ratio=0.75)
        args.update(kw)
        with pytest.raises(exc, match=word):
            sa.SetCriterion(**args)(outputs, targets)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        m(outputs, targets)


def test_matcher_draws_one_point_set_per_image_in_order():
    import streamformer_amd as sa
    arrays = [np.full((1, 5, 2), 0.1 * (i + 1), np.float32) for i in range(3)]
    q = CO.Queue(arrays)
    pts = sa.HungarianMatcher(num_points=5, rand=q).draw_points(3, "cpu")
    assert q.shapes == [(1, 5, 2)] * 3 and q.done() and pts.shape == (3, 5, 2)
    assert torch.equal(pts[:, 0, 0], torch.tensor([0.1, 0.2, 0.3]))
    with pytest.raises(ValueError, match="draw"):
        sa.HungarianMatcher(num_points=5, rand=lambda shape, device: torch.zeros(2, 2)).draw_points(1, "cpu")


def test_pair_table_and_assignment_on_the_host():
    from streamformer_amd import criterion as K
    cost = np.zeros((2, 2, 3, 2), np.float32)
    cost[0, 0] = [[5, 1], [0, 5], [5, 5]]
    cost[1, 0] = [[5, 5], [5, 0], [1, 5]]
    idx = K.assign(cost, [2, 0])
    assert [t.tolist() for t in idx[0][0]] == [[0, 1], [1, 0]] and [t.tolist() for t in idx[1][0]] == [[1, 2], [1, 0]]
    assert idx[0][1][0].numel() == 0 and idx[0][1][0].dtype == torch.int64 and idx[0][0][0].device.type == "cpu"
    pairs, start = K.pair_table(idx)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 0, 0, 1], [0, 0, 1, 0], [1, 0, 1, 1], [1, 0, 2, 0]] and start == [0, 2, 4]
    assert K.pair_table([[(np.zeros(0), np.zeros(0))]])[0].shape == (0, 4)
    with pytest.raises(ValueError):
        K.pair_table([[(np.zeros(2), np.zeros(1))]])


def test_num_masks_and_keys():
    from streamformer_amd import criterion as K
    t = lambda n: {"labels": torch.zeros(n, dtype=torch.int64)}      # noqa: E731
    assert K._num_masks([t(3), t(0), t(5)], "cpu") == 8.0 and K._num_masks([t(0)], "cpu") == 1.0 and K._num_masks([], "cpu") == 1.0
    assert CO.loss_names(2) == [("loss_ce", "loss_mask", "loss_dice"), ("loss_ce_0", "loss_mask_0", "loss_dice_0")]
    assert CO.loss_names(1, "vis")[0] == ("vis_loss_ce", "vis_loss_mask", "vis_loss_dice")
    layers = K._layers_of({"pred_logits": 1, "pred_masks": 2, "aux_outputs": [{"pred_logits": 3, "pred_masks": 4}]})
    assert layers == [{"pred_logits": 1, "pred_masks": 2}, {"pred_logits": 3, "pred_masks": 4}]
