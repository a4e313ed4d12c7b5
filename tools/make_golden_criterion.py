"""Fixture F27 (tests/golden/f27_criterion.npz): the reference's own ``SetCriterion`` and ``HungarianMatcher``
(downstream/OVIS/mask2former/modeling/criterion.py, matcher.py) in fp64 on the CPU over the planted scenario of tests/criterion_oracle.py.

    python tools/make_golden_criterion.py /path/to/reference [--check]

``--check`` runs every comparison and writes nothing.  The cases of ``criterion_oracle.EXTRA`` (too large to store) go through the same
comparisons with the reference; only their results are not kept.

The path argument is only imported from (never on the GPU machine; nothing of the reference is stored).  detectron2 is not needed: as in
tools/make_golden_seg.py, stand-ins written from the call sites are registered for ``detectron2.utils.comm.get_world_size`` (1) and for the
two ``point_rend`` functions, which are a few lines each: ``point_sample`` is ``F.grid_sample`` at ``2 p - 1`` with a unit axis added and
removed, ``get_uncertain_point_coords_with_randomness`` draws ``[N, int(K * oversample), 2]`` points, keeps the ``int(importance * K)`` of
largest uncertainty by ``torch.topk`` and appends ``[N, K - that, 2]`` fresh draws when that is positive.  The packages above the two files
are namespace modules, so that their detectron2-importing ``__init__`` files never run (``utils/misc.py`` is the reference's own; a bare
``torchvision`` module stands in when torchvision is absent).  For the duration of a call ``torch.rand`` is replaced by the queue of planted
draws (tests/criterion_oracle.py ``draws``: the fixture stores them), and ``Tensor.float`` by the identity, so that the matcher's
``.float()`` casts leave the fp64 inputs in fp64.  The four scripted loss functions run as they are.

Before anything is written the generator checks (and tests/test_criterion_cpu.py checks again) the three conditions of the scenario:
the oracle agrees with the reference exactly on every assignment and chosen index set and to 1e-12 on every cost and loss; every
assignment has a margin of at least 1e-3 of the largest |cost| against forbidding any one of its pairs, and the fp32 oracle assigns as the
fp64 one; at most 1e-2 of a pair's chosen points are undecided, and the fp32 oracle's chosen sets differ from the fp64 ones only there.
Stored per case: a checksum of the inputs, the draws (fp32), per (layer, image) the cost matrix (fp64) and the indices, per layer the
chosen indices, the losses [L, 3] (fp64); and the measured margin and undecided share.
"""
import importlib
import importlib.machinery
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import criterion_oracle as CO      # noqa: E402

PKG = ("downstream", "OVIS", "mask2former")
OUT = os.path.join(ROOT, "tests", "golden", "f27_criterion.npz")


def _module(name, package=False, path=None, **attrs):
    m = types.ModuleType(name)
    if package:
        m.__path__ = [path] if path else []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def point_sample(input, point_coords, **kwargs):
    add_dim = point_coords.dim() == 3
    if add_dim:
        point_coords = point_coords.unsqueeze(2)
    output = F.grid_sample(input, 2.0 * point_coords - 1.0, **kwargs)
    return output.squeeze(3) if add_dim else output


def get_uncertain_point_coords_with_randomness(coarse_logits, uncertainty_func, num_points, oversample_ratio, importance_sample_ratio):
    assert oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1
    n, sampled = coarse_logits.shape[0], int(num_points * oversample_ratio)
    coords = torch.rand(n, sampled, 2, device=coarse_logits.device, dtype=coarse_logits.dtype)
    uncertainty = uncertainty_func(point_sample(coarse_logits, coords, align_corners=False))
    uncertain = int(importance_sample_ratio * num_points)
    idx = torch.topk(uncertainty[:, 0, :], k=uncertain, dim=1)[1]
    coords = torch.gather(coords, 1, idx[:, :, None].expand(n, uncertain, 2))
    if num_points - uncertain > 0:
        coords = torch.cat([coords, torch.rand(n, num_points - uncertain, 2, device=coarse_logits.device)], dim=1)
    return coords


def _load_reference(ref_root):
    _module("detectron2", package=True)
    _module("detectron2.utils", package=True)
    _module("detectron2.utils.comm", get_world_size=lambda: 1)
    _module("detectron2.projects", package=True)
    _module("detectron2.projects.point_rend", package=True)
    _module("detectron2.projects.point_rend.point_features", point_sample=point_sample,
            get_uncertain_point_coords_with_randomness=get_uncertain_point_coords_with_randomness)
    try:
        import torchvision  # noqa: F401
    except Exception:
        _module("torchvision", _is_tracing=lambda: False)
    for i in range(len(PKG)):
        _module(".".join(PKG[:i + 1]), package=True, path=os.path.join(ref_root, *PKG[:i + 1]))
    name = ".".join(PKG)
    _module(name + ".modeling", package=True, path=os.path.join(ref_root, *PKG, "modeling"))
    _module(name + ".utils", package=True, path=os.path.join(ref_root, *PKG, "utils"))
    sys.path.insert(0, ref_root)
    return importlib.import_module(name + ".modeling.criterion"), importlib.import_module(name + ".modeling.matcher")


class _Planted:
    """torch.rand -> the queue, Tensor.float -> identity, for the duration of a ``with``; records what the reference chose."""

    def __init__(self, queue):
        self.queue, self.chosen = queue, []

    def __enter__(self):
        self.rand, self.float, self.topk = torch.rand, torch.Tensor.float, torch.topk
        torch.rand = lambda *size, device=None, dtype=None, **kw: self.queue(size[0] if len(size) == 1 and not isinstance(size[0], int) else size, device)
        torch.Tensor.float = lambda t, *a, **k: t

        def topk(*a, **k):
            out = self.topk(*a, **k)
            self.chosen.append(out[1].clone())
            return out
        torch.topk = topk
        return self

    def __exit__(self, *exc):
        torch.rand, torch.Tensor.float, torch.topk = self.rand, self.float, self.topk


def reference_run(crit_mod, match_mod, case):
    matcher = match_mod.HungarianMatcher(cost_class=case["w_class"], cost_mask=case["w_mask"], cost_dice=case["w_dice"], num_points=case["K"])
    costs, indices = [], []
    solve = match_mod.linear_sum_assignment

    def recording(C):
        costs.append(C.clone().double())
        out = solve(C)
        indices.append((np.asarray(out[0], np.int64), np.asarray(out[1], np.int64)))
        return out
    match_mod.linear_sum_assignment = recording
    crit = crit_mod.SetCriterion(case["C"], matcher, {}, case["eos"], ["labels", "masks"], case["K"], case["over"], case["imp"]).double()
    outputs, targets, _ = CO.tensors(case, torch.float64)
    queue = CO.Queue(CO.draws(case), torch.float64)
    try:
        with _Planted(queue) as planted:
            losses = crit(outputs, targets)
    finally:
        match_mod.linear_sum_assignment = solve
    assert queue.done(), "the reference made fewer draws than planted"
    B = case["B"]
    return dict(costs=[costs[l * B:(l + 1) * B] for l in range(case["L"])], indices=[indices[l * B:(l + 1) * B] for l in range(case["L"])],
                chosen=planted.chosen, losses=torch.stack([torch.stack([losses[k].double() for k in names]) for names in CO.loss_names(case["L"])]))


def check_and_pack(name, case, ref, store):
    o64, o32 = CO.run(case, torch.float64), CO.run(case, torch.float32)
    K, KO, KU, KR = CO.counts(case)
    margin, share = float("inf"), 0.0
    for l in range(case["L"]):
        for b in range(case["B"]):
            assert float((o64["costs"][l][b] - ref["costs"][l][b]).abs().max() if ref["costs"][l][b].numel() else 0.0) <= 1e-12, (name, l, b)
            for got, got32, want in zip(o64["indices"][l][b], o32["indices"][l][b], ref["indices"][l][b]):
                assert np.array_equal(got.numpy(), want) and np.array_equal(got32.numpy(), want), (name, l, b)
            margin = min(margin, CO.assignment_margin(ref["costs"][l][b].numpy()))
            store[f"{name}_cost_{l}_{b}"] = ref["costs"][l][b].numpy()
            store[f"{name}_src_{l}_{b}"], store[f"{name}_tgt_{l}_{b}"] = ref["indices"][l][b]
        assert torch.equal(o64["chosen"][l].sort(1).values, ref["chosen"][l].sort(1).values), (name, l)      # pair by pair, in pair order
        und = CO.undecided(o64["x_over"][l], o32["x_over"][l], KU)
        if KU:
            share = max(share, float(und.sum(1).max()) / KU)
        assert CO.differs_only_in(o32["chosen"][l], o64["chosen"][l], und), (name, l)
        store[f"{name}_chosen_{l}"] = ref["chosen"][l].sort(1).values.numpy().astype(np.int32)
    assert float((o64["losses"] - ref["losses"]).abs().max()) <= 1e-12, (name, (o64["losses"] - ref["losses"]).abs())
    assert margin >= CO.MARGIN_REL, (name, margin)
    assert share <= CO.CAP, (name, share)
    store[f"{name}_losses"] = ref["losses"].numpy()
    store[f"{name}_checksum"] = CO.checksum(case)
    for i, d in enumerate(CO.draws(case)):
        store[f"{name}_draw_{i}"] = d
    return margin, share


def main():
    warnings.simplefilter("ignore")
    crit_mod, match_mod = _load_reference(os.path.abspath(sys.argv[1]))
    store, margin, share = {}, float("inf"), 0.0
    for name, case in list(CO.CASES.items()) + list(CO.EXTRA.items()):
        stored = name in CO.CASES                              # the cases beside the fixture meet the same checks; nothing of them is kept
        ref = reference_run(crit_mod, match_mod, case)
        if CO.counts(case)[2] == 0:
            ref["chosen"] = [torch.zeros(CO.pairs_per_layer(case), 0, dtype=torch.int64) for _ in range(case["L"])]
        m, s = check_and_pack(name, case, ref, store if stored else {})
        print(f"{name}{'' if stored else ' (not stored)'}: assignment margin {m:.3e}, undecided share {s:.3e}, losses {ref['losses'].flatten().tolist()}")
        if stored:
            margin, share = min(margin, m), max(share, s)
    store["margin"], store["undecided_share"] = np.asarray(margin), np.asarray(share)
    if "--check" in sys.argv:
        print(f"checked, nothing written: margin {margin:.3e}, undecided share {share:.3e}")
        return
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): margin {margin:.3e}, undecided share {share:.3e}")


if __name__ == "__main__":
    main()
