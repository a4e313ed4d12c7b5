"""CPU: the CTVIS contrastive-loss oracle (tests/cl_plugin_oracle.py) against fixture F28 = the reference's own CTCLPlugin in fp64, the
conditions on the planted scenario (every branch taken, the |sim| margin, fp32 taking the same beta branches), and the host-side logic of
streamformer_amd/cl_plugin.py that needs no device: the plan builder, the refusals, the key handling of ``ctvis_train_losses``."""
import os
import random

import numpy as np
import pytest
import torch

from tests import cl_plugin_oracle as PO
from tests import criterion_oracle as CO
from tests.helpers import load_npz

ALL = dict(PO.CASES, e2e=PO.E2E)
NAMES = sorted(ALL)
_RUNS = {}


def oracle(name, dtype):
    if (name, dtype) not in _RUNS:
        _RUNS[name, dtype] = PO.run(ALL[name], dtype, grad=dtype == torch.float64)
    return _RUNS[name, dtype]


@pytest.fixture(scope="module")
def f28(golden_dir):
    return load_npz(os.path.join(golden_dir, "f28_cl_plugin.npz"))


def test_scenario_shapes_are_the_planted_ones():
    shapes = {(c["F"], c["Q"], c["nn"], c["C"]) for c in ALL.values()}
    assert {s[0] for s in shapes} == {1, 2, 5} and {s[1] for s in shapes} == {8, 12} and {s[2] for s in shapes} == {7, 9} and {s[3] for s in shapes} == {256, 40}
    assert all(c["B"] == 2 for c in ALL.values())
    assert PO.CASES["tight"]["Q"] == PO.CASES["tight"]["nn"] + 1 and PO.CASES["main"]["Q"] > PO.CASES["main"]["nn"] + 1
    assert PO.instances(PO.CASES["tight"], 1) == 0 and "00000" in PO.CASES["main"]["valid"][0] and not PO.CASES["nomom"]["momentum"]
    assert PO.exist_after([False, True, False, True, True], 1) is False and PO.exist_after([False, True, False, False, False], 1) is True      # the quirk


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_the_reference(f28, name):
    """Plans and labels exactly, every float within 1e-12; the gradient is the reference's autograd's."""
    case, o = ALL[name], oracle(name, torch.float64)
    assert np.array_equal(PO.checksum(case), f28[f"{name}_checksum"]), "the scenario is not the one the fixture was made from"
    items, neg, start = PO.plan_arrays(o["plan"])
    assert np.array_equal(items, f28[f"{name}_items"]) and np.array_equal(neg, f28[f"{name}_neg"]) and np.array_equal(start, f28[f"{name}_neg_start"])
    if o["items"]:
        dot = np.concatenate([d.detach().numpy().reshape(-1) for d, _, _ in o["items"]])
        cos = np.concatenate([c.detach().numpy().reshape(-1) for _, c, _ in o["items"]])
        label = np.concatenate([y.numpy().reshape(-1) for _, _, y in o["items"]])
        assert np.array_equal(label, f28[f"{name}_label"])
        assert float(np.abs(dot - f28[f"{name}_dot"]).max()) <= 1e-12 and float(np.abs(cos - f28[f"{name}_cos"]).max()) <= 1e-12
    else:
        assert f28[f"{name}_dot"].size == 0
    got, want = PO.sg_array(case, o["sg"]), f28[f"{name}_sg"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and float(np.nanmax(np.abs(got - want), initial=0.0)) <= 1e-12
    assert float(np.abs(np.asarray([float(v.detach()) for v in o["losses"]]) - f28[f"{name}_losses"]).max()) <= 1e-12
    assert float(np.abs(np.asarray([float(o["weighted"][k].detach()) for k in ("loss_reid", "loss_aux_reid")]) - f28[f"{name}_weighted"]).max()) <= 1e-12
    assert float(np.abs(o["embeds"].grad.numpy() - f28[f"{name}_grad"]).max()) <= 1e-12
    assert np.array_equal(np.asarray([o["counts"][k] for k in PO.BRANCHES]), f28[f"{name}_counts"])


def test_every_branch_is_taken_and_sims_keep_their_margin(f28):
    total = sum(f28[f"{name}_counts"] for name in NAMES)
    assert not [k for k, v in zip(PO.BRANCHES, total) if v == 0]
    for name in NAMES:
        o = oracle(name, torch.float64)
        negative = [k for k, v in o["sim"].items() if float(v.detach()) < 0]
        assert set(negative) == set(ALL[name]["flip"])
        assert PO.min_abs_sim(o["sim"], skip=negative) >= PO.SIM_MARGIN and float(f28[f"{name}_min_abs_sim"]) >= PO.SIM_MARGIN
    assert len(PO.CASES["main"]["flip"]) == 1
    assert oracle("single", torch.float64)["plan"] == [] and float(oracle("single", torch.float64)["total"]) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_fp32_oracle_takes_the_same_branches(name):
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    assert o32["plan"] == o64["plan"] and set(o32["sim"]) == set(o64["sim"])
    assert all((o32["sim"][k] > 0) == (o64["sim"][k] > 0) for k in o64["sim"])


def test_end_to_end_scenario_assigns_with_margin(f28):
    """The masks and logits of the end-to-end scenario give assignments with the margin tests/criterion_oracle.py demands, in fp32 as in fp64."""
    i64, c64 = PO.matcher_indices(PO.E2E, torch.float64)
    i32, _ = PO.matcher_indices(PO.E2E, torch.float32)
    for f in range(PO.E2E["F"]):
        for b in range(PO.E2E["B"]):
            assert CO.assignment_margin(c64[f][b].numpy()) >= CO.MARGIN_REL, (f, b)
            assert all(torch.equal(a, c) for a, c in zip(i64[f][b], i32[f][b]))


# ---------------------------------------------------------------------------------------------------
# host-side logic of the module
# ---------------------------------------------------------------------------------------------------
def targets_list(case):
    """prepare_targets' result for a scenario, on the CPU."""
    valid = PO.valid_flags(case)
    return [[{"valid": torch.tensor(valid[b][f], dtype=torch.bool)} for b in range(case["B"])] for f in range(case["F"])]


@pytest.mark.parametrize("name", NAMES)
def test_host_plan_reproduces_the_fixture(f28, name):
    """The plan builder on the fixture's indices with the reference's seeding: F28's plan draw for draw, and a consistent table."""
    import streamformer_amd as sa
    case = ALL[name]
    plugin = sa.CTCLPlugin(weight_dict=PO.WEIGHTS, num_negatives=case["nn"], sampling_frame_num=case["F"], momentum_embed=case["momentum"])
    random.seed(case["draw_seed"])
    np.random.seed(case["draw_seed"])
    plan = plugin.plan(targets_list(case), PO.scripted_indices(case), case["Q"])
    items, neg, start = PO.plan_arrays(plan.items)
    assert np.array_equal(items, f28[f"{name}_items"]) and np.array_equal(neg, f28[f"{name}_neg"]) and np.array_equal(start, f28[f"{name}_neg_start"])
    assert plan.tracks == PO.track_ids(case) and plan.I == len(items) and plan.NE == len(neg) and plan.table.dtype == np.int32
    Fn, Q, R = case["F"], case["Q"], case["B"] * case["F"] * case["Q"]
    o = plan.offsets
    rows, titems = plan.table[o[0]:o[1]].reshape(-1, Fn), plan.table[o[1]:o[2]].reshape(-1, Fn)
    rec, negs = plan.table[o[2]:o[3]].reshape(-1, 8), plan.table[o[3]:o[4]]
    row_start, row_items = plan.table[o[4]:o[5]], plan.table[o[5]:o[5] + plan.NE]
    assert row_start.size == R + 1 and row_start[0] == 0 and row_start[-1] == plan.NE and (np.diff(row_start) >= 0).all()
    assert ((rows >= -1) & (rows < R)).all() and ((negs >= 0) & (negs < R)).all() and ((row_items >= 0) & (row_items < max(plan.I, 1))).all()
    for n, (b, i, f, q, kind, pf) in enumerate(items):
        t = plan.tracks.index((b, i))
        assert titems[t, f] == n and rec[n, 2] == (b * Fn + f) * Q + q == rows[t, f] and rec[n, 7] == pf
        assert rec[n, 4] == (t * Fn + pf if kind else rows[t, pf]) and rec[n, 4] >= 0
        mine = negs[rec[n, 5]:rec[n, 5] + rec[n, 6]]
        assert np.array_equal(mine, (b * Fn + f - 1) * Q + neg[start[n]:start[n + 1]])
        assert all(n in row_items[row_start[r]:row_start[r + 1]] for r in mine)
    for r in range(R):                                        # a row's items in plan order
        assert (np.diff(row_items[row_start[r]:row_start[r + 1]]) > 0).all()


def test_hooks_are_called_in_the_references_order():
    import streamformer_amd as sa
    case, calls = PO.CASES["tight"], []

    def sample(population, k):
        calls.append(("sample", len(population), k))
        return list(population)[:k]

    def coin():
        calls.append(("coin",))
        return 0.75
    plugin = sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=5, sample=sample, coin=coin)
    plan = plugin.plan(targets_list(case), PO.scripted_indices(case), 8)
    # video 0: 9 valid (frame, instance) cells filled first, then one coin per item with an earlier present frame ("00100" has none)
    assert calls == [("sample", 7, 7)] * 9 + [("coin",)] * 6 and all(it[4] == 1 for it in plan.items) and plan.I == 6
    assert sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=5, momentum_embed=False, coin=coin).plan(
        targets_list(case), PO.scripted_indices(case), 8).I == 6 and len(calls) == 15


class _Inst:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_prepare_targets_takes_instances_and_dicts():
    import streamformer_amd as sa
    plugin = sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=2)
    masks = torch.zeros(2, 4, 4)
    a = _Inst(image_size=(4, 4), gt_classes=torch.tensor([3, 1]), gt_masks=_Inst(tensor=masks), gt_ids=torch.tensor([5, -1]))
    b = {"labels": torch.tensor([3, 1]), "masks": masks, "ids": torch.tensor([-1, 7])}
    out = plugin.prepare_targets([a, b, b, a])
    assert len(out) == 2 and len(out[0]) == 2 and out[0][0]["valid"].tolist() == [True, False] and out[1][0]["valid"].tolist() == [False, True]
    assert out[0][1]["valid"].tolist() == [False, True] and out[0][0]["masks"] is masks and set(out[0][0]) == {"labels", "masks", "inst_id", "valid"}
    with pytest.raises(ValueError, match="multiple"):
        plugin.prepare_targets([a, b, b])


def test_refusals_need_no_device():
    import streamformer_amd as sa
    with pytest.raises(NotImplementedError, match="noise_embed"):
        sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=2, noise_embed=True)
    sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=2, bio_cl=True)            # accepted, without effect
    plugin = sa.CTCLPlugin(weight_dict={}, num_negatives=7, sampling_frame_num=2)
    t = lambda *counts: [[{"valid": torch.ones(c, dtype=torch.bool)}] for c in counts]      # noqa: E731  (one video, a count per frame)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        plugin._refuse(torch.zeros(2, 8, 40), t(1, 1))
    # a stand-in with a device tensor's device, shape and dim: the checks read nothing else
    fake = lambda *shape: type("T", (), {"device": torch.device("cuda"), "shape": torch.Size(shape), "dim": lambda self: len(shape)})()      # noqa: E731
    for shape, tl, exc, word in (((3, 8, 40), t(1, 1), ValueError, "sampling_frame_num"), ((2, 8, 40), t(1, 2), ValueError, "differing"),
                                 ((2, 8, 40), t(9, 9), ValueError, "instances for"), ((2, 7, 40), t(1, 1), ValueError, "num_negatives"),
                                 ((2, 8, 36), t(1, 1), RuntimeError, "capacity"), ((2, 8, 264), t(1, 1), RuntimeError, "capacity")):
        with pytest.raises(exc, match=word):
            plugin._refuse(fake(*shape), tl)
    with pytest.raises(ValueError, match="two present"):
        sa.cl_plugin.Plan([[[3, 3]]], [[[True, True]]], 1, 8, 7)


def test_ctvis_train_losses_keys():
    import streamformer_amd as sa

    class Crit:
        weight_dict = {"loss_ce": 2.0, "loss_mask": 5.0}
        matcher = "the matcher"

        def __call__(self, outputs, targets):
            return {"loss_ce": torch.tensor(1.0), "loss_mask": torch.tensor(2.0), "loss_other": torch.tensor(9.0)}

    class Plug:
        def train_loss(self, outputs, gt, matcher):
            assert matcher == "the matcher" and gt == "gt"
            return {"loss_reid": torch.tensor(0.5)}
    out = sa.ctvis_train_losses({}, [], "gt", Crit(), Plug())
    assert list(out) == ["loss_ce", "loss_mask", "loss_reid"] and [float(v) for v in out.values()] == [2.0, 10.0, 0.5]
