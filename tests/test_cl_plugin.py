"""GPU: the native CTVIS contrastive loss (streamformer_amd/cl_plugin.py, csrc/sf_cl_plugin.hip) against tests/cl_plugin_oracle.py and
fixture F28 (the reference's own CTCLPlugin in fp64).  Bounds are tests/helpers.py ``check_against_floor``: MARGIN (4) x the error
against fp64 of the same operator sequence in torch fp32.  Every test prints error over bound; the largest ratio measured on the MI355X
stands in each test's docstring."""
import os

import numpy as np
import pytest
import torch

import streamformer_amd as sa
from streamformer_amd import cl_plugin as CP
from streamformer_amd import criterion as K
from tests import cl_plugin_oracle as PO
from tests import criterion_oracle as CO
from tests.helpers import NoLaunch, check_against_floor, gpu_device, guarded, load_npz, read_guarded

pytestmark = pytest.mark.gpu

ALL = dict(PO.CASES, e2e=PO.E2E)
WITH_ITEMS = ["main", "tight", "nomom", "e2e"]
_RUNS = {}


def oracle(name, dtype):
    if (name, dtype) not in _RUNS:
        _RUNS[name, dtype] = PO.run(ALL[name], dtype, grad=True)
    return _RUNS[name, dtype]


@pytest.fixture(scope="module")
def f28(golden_dir):
    return load_npz(os.path.join(golden_dir, "f28_cl_plugin.npz"))


def targets_list(case):
    valid = PO.valid_flags(case)
    return [[{"valid": torch.tensor(valid[b][f], dtype=torch.bool)} for b in range(case["B"])] for f in range(case["F"])]


def seeded_plugin(case, **kw):
    sample, coin = PO.seeded_hooks(case["draw_seed"])
    return sa.CTCLPlugin(weight_dict=dict(PO.WEIGHTS), num_negatives=case["nn"], sampling_frame_num=case["F"], momentum_embed=case["momentum"],
                         sample=sample, coin=coin, **kw)


def native_step(name, dev):
    """(step, embeds): the plan of the scenario with the reference's draws, on the device."""
    case = ALL[name]
    e = torch.tensor(PO.embeddings(case), device=dev).flatten(0, 1).contiguous()
    plan = seeded_plugin(case).plan(targets_list(case), PO.scripted_indices(case), case["Q"])
    assert plan.items == oracle(name, torch.float64)["plan"]
    return CP._Step(plan, e), e


def per_item(items):
    """(contras, aux) per item of an oracle run, in its dtype."""
    c = [torch.logsumexp(torch.nn.functional.pad(d[1:, 0] - d[0, 0], (0, 1)), 0) for d, _, _ in items]
    a = [((cos[:, 0] - y) ** 2).mean() for _, cos, y in items]
    return torch.stack(c).detach(), torch.stack(a).detach()


@pytest.mark.parametrize("name", WITH_ITEMS)
def test_tracks_alone(name):
    """sf_op_clp_tracks: sg, sim and beta per (instance, frame) inside the bound; where sim < 0, beta is exactly 0 and sg repeats bit for
    bit; absent frames repeat bit for bit; zeros before the first present frame.  Largest error over bound measured: 0.74 (sim and beta, F = 2), 0.32 (sg)."""
    dev, case = gpu_device(), ALL[name]
    step, e = native_step(name, dev)
    T, Fn, C = step.plan.T, case["F"], case["C"]
    b_sg, v_sg = guarded(dev, T, Fn, C)
    b_st, v_st = guarded(dev, T, Fn, 2)
    step.tracks(e, sg=v_sg, stats=v_st)
    sg, st = read_guarded(b_sg, v_sg), read_guarded(b_st, v_st)
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    w64, w32 = torch.from_numpy(PO.sg_array(case, o64["sg"])), torch.from_numpy(PO.sg_array(case, o32["sg"]))
    none = torch.isnan(w64)
    assert (sg[none] == 0).all()
    check_against_floor(f"{name} sg", sg[~none], w32[~none], w64[~none])
    keys = sorted(o64["sim"])
    if keys:
        ids = PO.track_ids(case)
        got = torch.stack([st[ids.index((b, i)), f] for b, i, f in keys])
        s64, s32 = (torch.stack([o["sim"][k].detach() for k in keys]) for o in (o64, o32))
        check_against_floor(f"{name} sim", got[:, 0], s32, s64)
        check_against_floor(f"{name} beta", got[:, 1], s32.clamp(min=0), s64.clamp(min=0))
        for (b, i, f), s in zip(keys, s64):
            if s < 0:
                t = ids.index((b, i))
                assert float(got[keys.index((b, i, f)), 1]) == 0.0 and torch.equal(sg[t, f].view(torch.int32), sg[t, f - 1].view(torch.int32))
    valid = PO.valid_flags(case)
    for t, (b, i) in enumerate(PO.track_ids(case)):
        for f in range(1, Fn):
            if not valid[b][f][i]:
                assert torch.equal(sg[t, f].view(torch.int32), sg[t, f - 1].view(torch.int32)) and st[t, f].tolist() == [0.0, 0.0]
    assert set(case["flip"]) == {k for k in keys if float(o64["sim"][k].detach()) < 0}


@pytest.mark.parametrize("name", WITH_ITEMS)
def test_items_alone(name):
    """sf_op_clp_items: per-item contras and aux inside the bound (C = 256 and 40, n = num_negatives and n = Q), the guard rows intact.
    Largest error over bound measured: 0.36 (aux), 0.29 (contras), 0.25 (the two sums)."""
    dev, case = gpu_device(), ALL[name]
    step, e = native_step(name, dev)
    step.tracks(e)
    b_it, v_it = guarded(dev, step.plan.I, 4)
    b_out, v_out = guarded(dev, 2)
    step.losses(e, out=v_out, item_out=v_it)
    got, out = read_guarded(b_it, v_it), read_guarded(b_out, v_out)
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    (c64, a64), (c32, a32) = per_item(o64["items"]), per_item(o32["items"])
    check_against_floor(f"{name} contras per item", got[:, 0], c32, c64)
    check_against_floor(f"{name} aux per item", got[:, 1], a32, a64)
    check_against_floor(f"{name} losses", out, torch.stack(o32["losses"]).detach(), torch.stack(o64["losses"]).detach())
    sizes = {len(p[6]) for p in o64["plan"]}
    assert sizes <= {case["nn"], case["Q"]} and (name not in ("main", "tight") or sizes == {case["nn"], case["Q"]})


def test_item_with_a_dot_spread_that_overflows_a_naive_exp():
    """d_pos = -80, one negative at +80: exp(160) is past fp32, the loss (about 160) is not.  The fp32 oracle's logsumexp subtracts the
    maximum as the kernel does.  Largest error over bound measured: 0.13."""
    dev = gpu_device()
    rng = np.random.default_rng(77)
    C, Q = 40, 8
    e = (rng.standard_normal((2, Q, C)) * 0.3).astype(np.float32)
    u = rng.standard_normal(C)
    a = (u / np.linalg.norm(u) * np.sqrt(80.0)).astype(np.float32)
    e[1, 0], e[0, 0], e[0, 1] = a, -a, a                    # anchor (frame 1), positive (frame 0), one negative of frame 0
    g2q, valid = [[[0], [0]]], [[[True], [True]]]
    res = {dt: PO.reid_loss(torch.tensor(e, dtype=dt), 2, 7, g2q, valid, coin=lambda: 0.0) for dt in (torch.float64, torch.float32)}
    want = per_item(res[torch.float64]["items"])
    assert 159.0 < float(want[0][0]) < 161.0 and not np.isfinite(np.exp(np.float32(160.0)))
    plan = CP.Plan(g2q, valid, 2, Q, 7, coin=lambda: 0.0)
    assert plan.items == res[torch.float64]["plan"]
    ed = torch.tensor(e, device=dev).flatten(0, 1)
    step = CP._Step(plan, ed)
    out = step.forward(ed).cpu()
    got = step.item_out.cpu()
    assert torch.isfinite(got).all()
    check_against_floor("spread contras", got[:, 0], per_item(res[torch.float32]["items"])[0], want[0])
    check_against_floor("spread aux", got[:, 1], per_item(res[torch.float32]["items"])[1], want[1])
    check_against_floor("spread losses", out, torch.stack(res[torch.float32]["losses"]), torch.stack(res[torch.float64]["losses"]))
    g = step.backward(ed, torch.tensor([1.0, 1.0], device=dev)).cpu()
    assert torch.isfinite(g).all()


@pytest.mark.parametrize("name", WITH_ITEMS)
def test_losses_against_the_fixture(f28, name):
    """get_reid_loss on the fixture's indices: both losses against F28 inside the bound, two runs bit-identical.  Largest error over bound
    measured: 0.25."""
    dev, case = gpu_device(), ALL[name]
    e = torch.tensor(PO.embeddings(case), device=dev)
    outputs_list = [{"pred_embeds": e[f::case["F"]]} for f in range(case["F"])]
    runs = []
    for _ in range(2):
        losses = seeded_plugin(case).get_reid_loss(targets_list(case), outputs_list, PO.scripted_indices(case))
        runs.append(torch.stack([losses["loss_reid"], losses["loss_aux_reid"]]).cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    o32 = oracle(name, torch.float32)
    check_against_floor(f"{name} losses", runs[0], torch.stack(o32["losses"]).detach(), torch.from_numpy(f28[f"{name}_losses"]))


def test_no_item_gives_exact_zeros_connected_to_the_graph(monkeypatch):
    dev, case = gpu_device(), PO.CASES["single"]
    e = torch.tensor(PO.embeddings(case), device=dev, requires_grad=True)
    plugin = seeded_plugin(case)
    losses = plugin._reid(e, targets_list(case), PO.scripted_indices(case))
    assert list(losses) == ["loss_reid", "loss_aux_reid"] and all(float(v) == 0.0 and v.requires_grad for v in losses.values())
    sum(losses.values()).backward()
    assert e.grad is not None and float(e.grad.abs().max()) == 0.0


@pytest.mark.parametrize("name", WITH_ITEMS)
def test_backward(f28, name):
    """sf_op_clp_backward with upstream (2, 3) against F28's fp64 gradient inside the bound; two runs bit-identical; rows no item
    references exactly zero; written into guarded buffers; loss.backward() gives the same bits.  Largest error over bound measured: 0.28."""
    dev, case = gpu_device(), ALL[name]
    step, e = native_step(name, dev)
    step.forward(e)
    up = torch.tensor([PO.WEIGHTS["loss_reid"], PO.WEIGHTS["loss_aux_reid"]], device=dev)
    runs = []
    for _ in range(2):
        buf, view = guarded(dev, step.plan.R, case["C"])
        step.backward(e, up, grad=view)
        runs.append(read_guarded(buf, view))
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    want = torch.from_numpy(f28[f"{name}_grad"]).flatten(0, 1)
    o32 = oracle(name, torch.float32)
    check_against_floor(f"{name} grad_pred_embeds", runs[0], o32["embeds"].grad.flatten(0, 1), want)
    untouched = (want == 0).all(1)
    assert untouched.any() and (runs[0][untouched] == 0).all(), "a row no item references has a gradient"
    leaf = torch.tensor(PO.embeddings(case), device=dev, requires_grad=True)
    losses = seeded_plugin(case)._reid(leaf, targets_list(case), PO.scripted_indices(case))
    (losses["loss_reid"] * PO.WEIGHTS["loss_reid"] + losses["loss_aux_reid"] * PO.WEIGHTS["loss_aux_reid"]).backward()
    assert torch.equal(leaf.grad.flatten(0, 1).cpu().view(torch.int32), runs[0].view(torch.int32))


class ScriptedMatcher(torch.nn.Module):
    """The reference-style foreign matcher: hands out given indices, position by position."""

    def __init__(self, per_position):
        super().__init__()
        self.per_position, self.calls = per_position, 0

    def forward(self, outputs, targets):
        self.calls += 1
        return self.per_position[self.calls - 1]


def e2e_inputs(dev, ids_on_device):
    case = PO.E2E
    cc = PO.crit_case(case)
    outputs, targets, _ = CO.tensors(cc, torch.float32, dev)
    valid = PO.valid_flags(case)
    det = dict(outputs, pred_embeds=torch.tensor(PO.embeddings(case), device=dev, requires_grad=True))
    gt = []
    for b in range(case["B"]):
        for f in range(case["F"]):
            n = b * case["F"] + f
            ids = torch.tensor([i if valid[b][f][i] else -1 for i in range(PO.instances(case, b))], dtype=torch.int64)
            gt.append({"labels": targets[n]["labels"], "masks": targets[n]["masks"], "ids": ids.to(dev) if ids_on_device else ids})
    matcher = sa.HungarianMatcher(cc["w_class"], cc["w_mask"], cc["w_dice"], num_points=cc["K"], rand=CO.Queue(PO.match_draws(case)))
    return case, det, gt, matcher


@pytest.mark.parametrize("ids_on_device", [False, True])
def test_train_loss_end_to_end(f28, monkeypatch, ids_on_device):
    """train_loss with the native HungarianMatcher: the oracle's plan, the weighted losses against F28 inside the bound, ONE
    criterion._device_to_host, no other device-to-host copy (one more, of gt_ids, when they live on the device); the same bits with a
    scripted foreign matcher and with the matcher run in chunks of frame positions.  Largest error over bound measured: 0.005."""
    dev = gpu_device()
    case, det, gt, matcher = e2e_inputs(dev, ids_on_device)
    copies, synced, real = [], [], K._device_to_host
    monkeypatch.setattr(K, "_device_to_host", lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    for meth in ("cpu", "item", "tolist", "numpy"):
        def counting(self, *a, _real=getattr(torch.Tensor, meth), _name=meth, **k):
            if self.is_cuda:
                synced.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counting)
    plugin = seeded_plugin(case)
    plugin._trace = []
    losses = plugin.train_loss(det, gt, matcher)
    assert matcher.rand.done() and len(copies) == 1 and synced == (["cpu"] if ids_on_device else []), (copies, synced)
    monkeypatch.undo()
    o64, o32 = oracle("e2e", torch.float64), oracle("e2e", torch.float32)
    assert plugin._trace[0].plan.items == o64["plan"] and list(losses) == ["loss_reid", "loss_aux_reid"]
    got = torch.stack([losses["loss_reid"], losses["loss_aux_reid"]]).detach()
    want32 = torch.stack([o32["weighted"][k] for k in ("loss_reid", "loss_aux_reid")]).detach()
    check_against_floor("e2e weighted losses", got, want32, torch.from_numpy(f28["e2e_weighted"]))
    foreign = ScriptedMatcher(PO.scripted_indices(case))
    again = seeded_plugin(case).train_loss(det, gt, foreign)
    assert foreign.calls == case["F"] and all(torch.equal(again[k], losses[k]) for k in losses)
    monkeypatch.setattr(K, "MAX_IMAGES", 2)                  # one frame position per matcher call
    matcher.rand = CO.Queue(PO.match_draws(case))
    chunked = seeded_plugin(case).train_loss(det, gt, matcher)
    assert matcher.rand.done() and all(torch.equal(chunked[k], losses[k]) for k in losses)
    dropped = sa.CTCLPlugin(weight_dict={"loss_reid": 2.0}, num_negatives=case["nn"], sampling_frame_num=case["F"]).train_loss(det, gt, foreign.__class__(
        PO.scripted_indices(case)))
    assert list(dropped) == ["loss_reid"]


def test_refusals_before_any_launch(monkeypatch):
    """Every refusal by name, with the library's entry points closed and the matcher never asked."""
    dev = gpu_device()
    guard = NoLaunch(CP.nat)
    monkeypatch.setattr(CP, "nat", guard)
    monkeypatch.setattr(K, "nat", guard)
    matcher = ScriptedMatcher([])

    def call(F=2, Q=8, C=40, counts=(1, 1), images=2, device=dev, nn=7, **kw):
        det = {"pred_logits": torch.zeros(images, Q, 3, device=device), "pred_masks": torch.zeros(images, Q, 4, 4, device=device),
               "pred_embeds": torch.zeros(images, Q, C, device=device)}
        gt = [{"labels": torch.zeros(g, dtype=torch.int64, device=device), "masks": torch.zeros(g, 4, 4, device=device),
               "ids": torch.arange(g)} for g in counts]
        return sa.CTCLPlugin(weight_dict={}, num_negatives=nn, sampling_frame_num=F, **kw).train_loss(det, gt, matcher)
    for kw, exc, word in ((dict(device="cpu"), RuntimeError, "CPU tensors"), (dict(counts=(1, 1, 1), images=3), ValueError, "multiple"),
                          (dict(counts=(1, 2)), ValueError, "differing"), (dict(counts=(9, 9)), ValueError, "instances for"),
                          (dict(Q=7), ValueError, "num_negatives"), (dict(C=36), RuntimeError, "capacity"), (dict(C=264), RuntimeError, "capacity"),
                          (dict(noise_embed=True), NotImplementedError, "noise_embed")):
        with pytest.raises(exc, match=word):
            call(**kw)
    assert guard.calls == [] and matcher.calls == 0
