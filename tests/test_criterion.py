"""GPU: the native Mask2Former criterion (streamformer_amd/criterion.py, csrc/sf_criterion.hip) against tests/criterion_oracle.py and
fixture F27 (the reference's own SetCriterion / HungarianMatcher in fp64).  Bounds are tests/helpers.py ``check_against_floor``: MARGIN
(4) x the error against fp64 of the same operator sequence in torch fp32.  Measured on the MI355X (largest error over bound per test):
see the summary each test prints."""
import os

import numpy as np
import pytest
import torch

import streamformer_amd as sa
from streamformer_amd import _native as nat
from streamformer_amd import criterion as K
from tests import criterion_oracle as CO
from tests.helpers import NoLaunch, check_against_floor, gpu_device, load_npz, maxabs

pytestmark = pytest.mark.gpu

CASE_NAMES = sorted(CO.CASES)
ALL_CASES = dict(CO.CASES, **CO.EXTRA)
# the cost kernel's other paths: 25 chunks of points (capacity); 2 chunks, 2 query tiles and 2, 4, 8 target tiles (wide*)
COST_NAMES = CASE_NAMES + ["capacity", "wide2", "wide4", "wide8"]
LOSS_NAMES = CASE_NAMES + ["capacity", "empty_big"]
_RUNS = {}


def oracle(name, dtype, **kw):
    key = (name, dtype) if not kw else None
    if key is None or key not in _RUNS:
        r = CO.run(ALL_CASES[name], dtype, **kw)
        if key is None:
            return r
        _RUNS[key] = r
    return _RUNS[key]


@pytest.fixture(scope="module")
def f27(golden_dir):
    return load_npz(os.path.join(golden_dir, "f27_criterion.npz"))


def want_indices(f27, name, l, b):
    """The assignment of (layer, image): F27's where the case is in the fixture, else the fp64 oracle's (same margin conditions)."""
    if name in CO.CASES:
        return f27[f"{name}_src_{l}_{b}"], f27[f"{name}_tgt_{l}_{b}"]
    return tuple(t.numpy() for t in oracle(name, torch.float64)["indices"][l][b])


def split_draws(case, dev):
    """The planted draws per layer: match [B, K, 2], over [N, KO, 2], rnd [N, KR, 2] or None."""
    d, out, at = CO.draws(case), [], 0
    kr = CO.counts(case)[3]
    for _ in range(case["L"]):
        lay = dict(match=torch.cat([torch.from_numpy(a) for a in d[at:at + case["B"]]]).to(dev), over=torch.from_numpy(d[at + case["B"]]).to(dev))
        at += case["B"] + 1
        lay["rnd"] = torch.from_numpy(d[at]).to(dev) if kr else None
        at += 1 if kr else 0
        out.append(lay)
    return out


def native_batch(case, dev):
    outputs, targets, leaves = CO.tensors(case, torch.float32, dev, grad=True)
    return outputs, targets, leaves, K._Batch(K._layers_of(outputs), targets, "test")


def native_step(name, dev, indices=None):
    """A _Step over the oracle's (or the given) indices, with the planted draws, after its forward: (step, losses [L, 3])."""
    case = ALL_CASES[name]
    outputs, targets, leaves, batch = native_batch(case, dev)
    d = split_draws(case, dev)
    pairs, start = K.pair_table(indices or oracle(name, torch.float64)["indices"])
    k, ko, ku, kr = CO.counts(case)
    w = torch.ones(case["C"] + 1)
    w[-1] = case["eos"]
    step = K._Step(batch, pairs, start, max(float(sum(case["G"])), 1.0), True, True, w, k, ko, ku, torch.cat([x["over"] for x in d]).contiguous(),
                   torch.cat([x["rnd"] for x in d]).contiguous() if kr else None, debug=True)
    return step, step.forward()


def chosen_per_layer(step, case):
    ku, n = CO.counts(case)[2], CO.pairs_per_layer(case)
    got = step.chosen.cpu().long()[:, :ku]
    return [got[l * n:(l + 1) * n] for l in range(case["L"])]


@pytest.mark.parametrize("name", COST_NAMES)
def test_cost_matrices_alone(name):
    """sf_op_crit_costs: every cost matrix inside the bound; columns >= G_b and the guard row untouched; two runs bit-identical."""
    dev, case = gpu_device(), ALL_CASES[name]
    _, _, _, batch = native_batch(case, dev)
    coords = torch.stack([x["match"] for x in split_draws(case, dev)])
    n = batch.L * batch.B * batch.Q * batch.G_max
    runs = []
    for _ in range(2):
        buf = torch.full((n + 64,), float("nan"), device=dev)
        K._cost_matrices(batch, coords, case["K"], case["w_class"], case["w_mask"], case["w_dice"], cost=buf[:n].view(batch.L, batch.B, batch.Q, batch.G_max))
        runs.append(buf.cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
    assert torch.isnan(runs[0][n:]).all(), "the guard row was written"
    got = runs[0][:n].view(batch.L, batch.B, batch.Q, batch.G_max)
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    for l in range(case["L"]):
        for b, g in enumerate(case["G"]):
            assert torch.isnan(got[l, b, :, g:]).all(), "columns past the image's targets were written"
            if g:
                assert not torch.isnan(got[l, b, :, :g]).any()
                check_against_floor(f"{name} cost[{l}][{b}]", got[l, b, :, :g], o32["costs"][l][b], o64["costs"][l][b])


@pytest.mark.parametrize("name", COST_NAMES)
def test_matcher_indices_and_one_copy(f27, name, monkeypatch):
    """Indices equal to F27 (beside it: to the fp64 oracle's) for every (layer, image), G = 0 and Q < G included; exactly one
    device-to-host copy per call."""
    dev, case = gpu_device(), ALL_CASES[name]
    outputs, targets, _, _ = native_batch(case, dev)
    copies, real = [], K._device_to_host
    monkeypatch.setattr(K, "_device_to_host", lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    d = CO.draws(case)
    per_layer = case["B"] + 1 + (CO.counts(case)[3] > 0)
    queue = CO.Queue([a for l in range(case["L"]) for a in d[l * per_layer:l * per_layer + case["B"]]])
    m = sa.HungarianMatcher(case["w_class"], case["w_mask"], case["w_dice"], num_points=case["K"], rand=queue)
    with torch.no_grad():
        got = m.match_layers(K._layers_of(outputs), targets)
    assert queue.done() and len(copies) == 1, copies
    for l in range(case["L"]):
        for b in range(case["B"]):
            i, j = got[l][b]
            assert i.dtype == torch.int64 and i.device.type == "cpu"
            src, tgt = want_indices(f27, name, l, b)
            assert np.array_equal(i.numpy(), src) and np.array_equal(j.numpy(), tgt), (l, b)
    copies.clear()
    first = sa.HungarianMatcher(case["w_class"], case["w_mask"], case["w_dice"], num_points=case["K"], rand=CO.Queue(d[:case["B"]]))(outputs, targets)
    assert len(copies) == 1 and all(np.array_equal(first[b][0].numpy(), want_indices(f27, name, 0, b)[0]) for b in range(case["B"]))


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_mask_losses_alone(name):
    """sf_op_crit_losses: chosen sets equal to the oracle's outside undecided points (share <= CAP), loss terms inside the bound, two
    runs bit-identical; the capacity case (K = 12544, 37632 oversampled points: 155936 bytes of LDS) passes.  In "empty_big" the image
    without targets has the batch's largest masks, which the coordinates scale by all the same."""
    dev, case = gpu_device(), ALL_CASES[name]
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    step, out = native_step(name, dev)
    step2, out2 = native_step(name, dev)
    assert torch.equal(out.cpu().view(torch.int32), out2.cpu().view(torch.int32)) and torch.equal(step.coords.cpu(), step2.coords.cpu())
    ku = CO.counts(case)[2]
    for l, got in enumerate(chosen_per_layer(step, case)):
        und = CO.undecided(o64["x_over"][l], o32["x_over"][l], ku)
        if ku:
            share = float(und.sum(1).max()) / ku
            print(f"  {name} layer {l}: undecided share {share:.3e}")
            assert share <= CO.CAP
            assert (got[:, 1:] > got[:, :-1]).all(), "chosen points are not in index order"
        assert CO.differs_only_in(got, o64["chosen"][l], und)
    check_against_floor(f"{name} loss_mask, loss_dice", out[:, 1:], o32["losses"][:, 1:], o64["losses"][:, 1:])
    check_against_floor(f"{name} loss_ce", out[:, 0], o32["losses"][:, 0], o64["losses"][:, 0])


def test_capacity_is_refused_before_any_launch(monkeypatch):
    dev = gpu_device()
    cap = nat.lib.sf_op_crit_losses_capacity()
    assert cap >= 37632 and (cap + 1352) * 4 <= 160 * 1024      # values + histogram, scan and partials: inside the CU's LDS
    step, _ = native_step("q_lt_g", dev)
    b = step.batch
    ws = nat.scratch(nat.lib.sf_op_crit_losses_workspace_bytes(step.N), dev)
    out = torch.full((3,), float("nan"), device=dev)
    args = lambda ko: (b.c_masks, b.L, b.B, b.Q, b.H, b.W, b.c_tgt_masks, b.c_G, b.c_H, b.c_W, step.pairs.data_ptr(), step.c_start, step.N,      # noqa: E731
                       step.over.data_ptr(), nat.ptr(step.rnd), step.K, ko, step.K_uncertain, 1.0, out.data_ptr(), 3, step.coords.data_ptr(),
                       step.sums.data_ptr(), 0, ws.data_ptr(), ws.numel(), nat.current_stream_handle(dev))
    assert nat.lib.sf_op_crit_losses(*args(cap + 1)) == nat.SF_ERR_CAPACITY and b"LDS" in nat.lib.sf_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out.cpu()).all(), "something was launched"
    crit = sa.SetCriterion(7, sa.HungarianMatcher(num_points=8), {}, 0.1, ["masks"], cap + 1, 1.0, 0.75)
    outputs, targets, _ = CO.tensors(CO.CASES["q_lt_g"], torch.float32, dev)
    guard = NoLaunch(K.nat)
    monkeypatch.setattr(K, "nat", guard)
    with pytest.raises(RuntimeError, match="capacity"):
        crit(outputs, targets)
    assert guard.calls == []


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_mask_losses_teacher_forced_and_backward(name):
    """With the oracle evaluated on the point sets the GPU chose (the rule of tests/test_mask_decoder.py): the loss terms, and
    grad_pred_masks / grad_pred_logits of every layer against the fp64 oracle's autograd, inside the bound; rows of unmatched queries
    exactly zero."""
    dev, case = gpu_device(), ALL_CASES[name]
    step, out = native_step(name, dev)
    chosen = chosen_per_layer(step, case)
    up = torch.tensor(np.random.default_rng(7).uniform(0.5, 2.0, (case["L"], 3)))
    res = {}
    for dtype in (torch.float64, torch.float32):
        r = oracle(name, dtype, chosen=chosen, grad=True)
        (r["losses"] * up.to(dtype)).sum().backward()
        res[dtype] = r
    o64, o32 = res[torch.float64], res[torch.float32]
    check_against_floor(f"{name} teacher-forced losses", out, o32["losses"].detach(), o64["losses"].detach())
    g_masks = step.backward_masks(up[:, 1:].float().to(dev)).cpu()
    g_logits = (step.class_grad * up[:, 0].float().to(dev).reshape(-1, 1, 1, 1)).cpu()
    matched = torch.zeros(case["L"], case["B"], case["Q"], dtype=torch.bool)
    for l, layer in enumerate(o64["indices"]):
        for b, (src, _) in enumerate(layer):
            matched[l, b, src] = True
    assert (g_masks[~matched] == 0).all(), "an unmatched query's plane has a gradient"
    for l in range(case["L"]):
        check_against_floor(f"{name} grad_pred_masks[{l}]", g_masks[l], o32["leaves"][l][1].grad, o64["leaves"][l][1].grad)
        check_against_floor(f"{name} grad_pred_logits[{l}]", g_logits[l], o32["leaves"][l][0].grad, o64["leaves"][l][0].grad)


class FixedMatcher(torch.nn.Module):
    """A stand-in matcher: hands out given indices, layer by layer."""

    def __init__(self, per_layer):
        super().__init__()
        self.per_layer, self.calls = per_layer, 0

    def forward(self, outputs, targets):
        self.calls += 1
        return self.per_layer[self.calls - 1]


@pytest.mark.parametrize("name", ["main", "sizes"])
def test_set_criterion_end_to_end(f27, name):
    """SetCriterion.forward at both geometries: every key against F27 inside the bound, the draws in the reference's order,
    loss.backward() equal to the kernel-level gradients; native losses on a stand-in matcher's indices, used as given."""
    dev, case = gpu_device(), CO.CASES[name]
    o64, o32 = oracle(name, torch.float64), oracle(name, torch.float32)
    names = CO.loss_names(case["L"])
    queue = CO.Queue(CO.draws(case))
    crit = sa.SetCriterion(case["C"], sa.HungarianMatcher(case["w_class"], case["w_mask"], case["w_dice"], case["K"], rand=queue), {}, case["eos"],
                           ["labels", "masks"], case["K"], case["over"], case["imp"], rand=queue).to(dev)
    outputs, targets, leaves = CO.tensors(case, torch.float32, dev, grad=True)
    crit._trace = []
    losses = crit(outputs, targets)
    assert queue.done() and list(losses) == [k for row in names for k in row]
    got = torch.stack([torch.stack([losses[k] for k in row]) for row in names])
    assert float(np.abs(o64["losses"].numpy() - f27[f"{name}_losses"]).max()) <= 1e-12
    check_against_floor(f"{name} losses", got.detach(), o32["losses"], torch.from_numpy(f27[f"{name}_losses"]))
    up = torch.tensor(np.random.default_rng(9).uniform(0.5, 2.0, (case["L"], 3)), dtype=torch.float32, device=dev)
    (got * up).sum().backward()
    step, = crit._trace
    want_masks = step.backward_masks(up[:, 1:])
    for l, (lg, mk) in enumerate(leaves):
        assert torch.equal(lg.grad, step.class_grad[l] * up[l, 0])
        scale = float(want_masks[l].abs().max())
        assert maxabs(mk.grad, want_masks[l]) <= 1e-5 * scale          # float atomics: the order of a plane's sums differs from run to run
    # a stand-in matcher: the reversed pairing of what the oracle matched, used as given
    given = [[(src.flip(0), tgt) for src, tgt in layer] for layer in o64["indices"]]
    queue2 = CO.Queue([a for i, a in enumerate(CO.draws(case)) if i % (case["B"] + 2) >= case["B"]])      # the loss draws alone
    fixed = FixedMatcher(given)
    crit2 = sa.SetCriterion(case["C"], fixed, {}, case["eos"], ["labels", "masks"], case["K"], case["over"], case["imp"], rand=queue2).to(dev)
    crit2._trace = []
    with torch.no_grad():
        l2 = crit2(outputs, targets, name="vis")
    assert fixed.calls == case["L"] and queue2.done() and list(l2) == ["vis_" + k for row in names for k in row]
    assert crit2._trace[0].pairs.cpu().tolist() == K.pair_table(given)[0].tolist()
    got2 = torch.stack([torch.stack([l2["vis_" + k] for k in row]) for row in names])
    chosen = chosen_per_layer(crit2._trace[0], case)
    w64, w32 = (CO.run(case, dtype, indices=given, chosen=chosen)["losses"] for dtype in (torch.float64, torch.float32))
    check_against_floor(f"{name} losses on given indices", got2, w32, w64)


def test_set_criterion_refusals_and_empty_batches(monkeypatch):
    """Refusals by name before any launch (the library's entry points are closed while they are provoked); a batch without any target works as in the reference: empty indices, zero mask losses with zero
    gradients, every query labelled no-object."""
    dev = gpu_device()
    case = dict(CO.CASES["q_lt_g"], G=(0,), Q=6)
    outputs, targets, leaves = CO.tensors(case, torch.float32, dev, grad=True)
    m = sa.HungarianMatcher(num_points=16)
    assert [tuple(t.numel() for t in p) for p in m(outputs, targets)] == [(0, 0)]
    crit = sa.SetCriterion(case["C"], m, {}, 0.1, ["labels", "masks"], 16, 3.0, 0.75).to(dev)
    crit._trace = []
    losses = crit(outputs, targets)
    assert float(losses["loss_mask"].detach()) == 0.0 and float(losses["loss_dice"].detach()) == 0.0
    want = torch.nn.functional.cross_entropy(leaves[0][0].detach().double().cpu().transpose(1, 2), torch.full((1, 6), case["C"]), crit.empty_weight.double().cpu())
    assert abs(float(losses["loss_ce"].detach()) - float(want)) <= 1e-5 * abs(float(want))
    assert (crit._trace[0].target_classes.cpu() == case["C"]).all()
    sum(losses.values()).backward()
    assert float(leaves[0][1].grad.abs().max()) == 0.0 and float(leaves[0][0].grad.abs().max()) > 0.0
    cpu_outputs, cpu_targets, _ = CO.tensors(case, torch.float32)
    guard = NoLaunch(K.nat)
    monkeypatch.setattr(K, "nat", guard)
    for bad, exc, word in ((dict(losses=["boxes"]), ValueError, "boxes"), (dict(oversample_ratio=0.9), ValueError, "oversample_ratio"),
                           (dict(importance_sample_ratio=-0.1), ValueError, "importance_sample_ratio")):
        args = dict(num_classes=case["C"], matcher=m, weight_dict={}, eos_coef=0.1, losses=["labels", "masks"], num_points=16, oversample_ratio=3.0,
                    importance_sample_ratio=0.75)
        args.update(bad)
        with pytest.raises(exc, match=word):
            sa.SetCriterion(**args).to(dev)(outputs, targets)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        crit(cpu_outputs, cpu_targets)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        m(cpu_outputs, cpu_targets)
    assert guard.calls == []
