"""Fixture F28 (tests/golden/f28_cl_plugin.npz): the reference's own ``CTCLPlugin``, ``SimpleTrainMemory``, ``TrainTracklet`` and
``loss_reid`` (downstream/OVIS/ctvis/modeling/cl_plugin/ct_cl_plugin.py) in fp64 on the CPU over the planted scenario of
tests/cl_plugin_oracle.py.

    python tools/make_golden_cl_plugin.py /path/to/reference [--check]

``--check`` runs every comparison and writes nothing.  The path argument is only imported from; nothing of the reference is stored.
detectron2 is not needed: stand-ins written from the call sites are registered for ``detectron2.config.configurable`` (a decorator
that leaves ``__init__`` as it is: the plugin is built with explicit keywords), ``detectron2.structures.BitMasks`` (a holder of
``.tensor``) and ``detectron2.utils.registry.Registry`` (``register()`` as a decorator, ``get``).  The packages above the file are
namespace modules, so that their detectron2-importing ``__init__`` files never run; ``ctvis/utils/utils.py`` is the reference's own.
``device='cuda'`` is hard-coded in ``TrainTracklet.__init__`` and in the plugin's ``device`` property: for the duration of a call the
torch constructors that receive it (``torch.zeros``, ``torch.arange``, ``torch.as_tensor``) map it to the CPU.

The whole of ``train_loss`` runs per case, with a scripted matcher that hands out the scenario's indices per frame position and
``gt_instances`` objects as detectron2 makes them (``image_size``, ``gt_classes``, ``gt_boxes``, ``gt_masks``, ``gt_ids``): the slicing
into positions, the targets' bookkeeping, the bank, the items and ``loss_reid`` are all the reference's code.  ``loss_reid`` is wrapped
to record the items it receives and the unweighted losses, ``SimpleTrainMemory.empty`` to keep every video's tracklets.  The draws are
the reference's own after ``random.seed(s); np.random.seed(s)``.

Checked before anything is written (and again by tests/test_cl_plugin_cpu.py): the oracle equals the reference exactly on the plan and
the labels and to 1e-12 on every float; every branch of ``cl_plugin_oracle.BRANCHES`` is taken at least once over the cases; every
|sim| except the planted negative ones is at least ``SIM_MARGIN``.  Stored per case: a checksum of the inputs, the plan, every item's
``dot_product``, ``cosine_similarity`` and ``label``, sg per (instance, frame), the two losses unweighted and weighted, d loss / d
pred_embeds of the weighted sum by the reference's autograd, and the smallest |sim|.
"""
import importlib
import importlib.machinery
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cl_plugin_oracle as PO      # noqa: E402

PKG = ("downstream", "OVIS", "ctvis")
OUT = os.path.join(ROOT, "tests", "golden", "f28_cl_plugin.npz")


def _module(name, package=False, path=None, **attrs):
    m = types.ModuleType(name)
    if package:
        m.__path__ = [path] if path else []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class BitMasks:
    def __init__(self, tensor):
        self.tensor = tensor


class Registry(dict):
    def __init__(self, name):
        super().__init__()
        self.name = name

    def register(self):
        def deco(cls):
            self[cls.__name__] = cls
            return cls
        return deco


def configurable(init):
    return init


def _load_reference(ref_root):
    _module("detectron2", package=True)
    _module("detectron2.config", configurable=configurable)
    _module("detectron2.structures", BitMasks=BitMasks)
    _module("detectron2.utils", package=True)
    _module("detectron2.utils.registry", Registry=Registry)
    try:
        import torchvision.ops.boxes  # noqa: F401
    except Exception:                         # utils.py imports box_area and never calls it on this path
        _module("torchvision", package=True)
        _module("torchvision.ops", package=True)
        _module("torchvision.ops.boxes", box_area=lambda boxes: (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))
    for i in range(len(PKG)):
        _module(".".join(PKG[:i + 1]), package=True, path=os.path.join(ref_root, *PKG[:i + 1]))
    name = ".".join(PKG)
    _module(name + ".modeling", package=True, path=os.path.join(ref_root, *PKG, "modeling"))
    _module(name + ".modeling.cl_plugin", package=True, path=os.path.join(ref_root, *PKG, "modeling", "cl_plugin"))
    _module(name + ".utils", package=True, path=os.path.join(ref_root, *PKG, "utils"))
    own = importlib.import_module(name + ".utils.utils")
    sys.modules[name + ".utils"].box_xyxy_to_cxcywh = own.box_xyxy_to_cxcywh
    sys.path.insert(0, ref_root)
    return importlib.import_module(name + ".modeling.cl_plugin.ct_cl_plugin")


class _OnCpu:
    """'cuda' -> 'cpu' in the torch constructors the reference hands its hard-coded device to, for the duration of a ``with``."""
    NAMES = ("zeros", "arange", "as_tensor")

    def __enter__(self):
        self.real = {n: getattr(torch, n) for n in self.NAMES}
        for n, fn in self.real.items():
            def wrapped(*a, _fn=fn, **k):
                if "device" in k and torch.device(k["device"]).type == "cuda":
                    k["device"] = "cpu"
                return _fn(*a, **k)
            setattr(torch, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, fn in self.real.items():
            setattr(torch, n, fn)


class Instances:
    """What detectron2's ``Instances`` gives the plugin."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class ScriptedMatcher(torch.nn.Module):
    def __init__(self, per_position):
        super().__init__()
        self.per_position, self.calls, self.seen = per_position, 0, []

    def forward(self, outputs, targets):
        self.calls += 1
        self.seen.append((tuple(outputs["pred_embeds"].shape), [t["valid"].tolist() for t in targets]))
        return self.per_position[self.calls - 1]


def reference_run(mod, case):
    e = torch.tensor(PO.embeddings(case), dtype=torch.float64, requires_grad=True)
    indices, valid = PO.scripted_indices(case), PO.valid_flags(case)
    B, Fn, Q = case["B"], case["F"], case["Q"]
    gt = []
    for b in range(B):
        for f in range(Fn):
            g = PO.instances(case, b)
            ids = torch.tensor([i if valid[b][f][i] else -1 for i in range(g)], dtype=torch.int64)
            masks = torch.zeros(g, 4, 4, dtype=torch.bool)
            gt.append(Instances(image_size=(4, 4), gt_classes=torch.arange(g), gt_boxes=Instances(tensor=torch.zeros(g, 4)),
                                gt_masks=BitMasks(masks) if b % 2 else masks, gt_ids=ids))
    plugin = mod.CTCLPlugin(weight_dict=dict(PO.WEIGHTS), num_negatives=case["nn"], sampling_frame_num=Fn, bio_cl=False,
                            momentum_embed=case["momentum"], noise_embed=False)
    det = {"pred_logits": torch.zeros(B * Fn, Q, 2, dtype=torch.float64), "pred_embeds": e, "aux_outputs": [{"pred_logits": None}]}
    rec = dict(items=None, raw=None, banks=[])
    real_loss, real_empty = mod.loss_reid, mod.SimpleTrainMemory.empty

    def loss_reid(qd_items, outputs, reduce=False):
        out = real_loss(qd_items, outputs, reduce)
        rec["items"], rec["raw"] = list(qd_items), {k: v.detach().clone() for k, v in out.items()}
        return out

    def empty(self):
        if self.tracklets:
            rec["banks"].append(dict(self.tracklets))
        real_empty(self)
    mod.loss_reid, mod.SimpleTrainMemory.empty = loss_reid, empty
    matcher = ScriptedMatcher(indices)
    random.seed(case["draw_seed"])
    np.random.seed(case["draw_seed"])
    try:
        with _OnCpu():
            losses = plugin.train_loss(det, gt, matcher)
            rec["banks"].append(dict(plugin.train_memory_bank.tracklets))
    finally:
        mod.loss_reid, mod.SimpleTrainMemory.empty = real_loss, real_empty
    assert matcher.calls == Fn and all(shape == (B, Q, case["C"]) for shape, _ in matcher.seen)
    assert [v for _, v in matcher.seen] == [[valid[b][f] for b in range(B)] for f in range(Fn)], "the reference sliced the targets differently"
    (losses["loss_reid"] + losses["loss_aux_reid"]).backward()
    banks = [bk for bk in rec["banks"] if bk]
    sg = {}
    videos = [b for b in range(B) if PO.instances(case, b)]
    assert len(banks) == len(videos), (len(banks), videos)
    for b, bank in zip(videos, banks):
        for i, tr in bank.items():
            sg[(b, i)] = tr.similarity_guided_reid_embed_list
    return dict(items=rec["items"], raw=rec["raw"], weighted=losses, grad=e.grad.detach(), sg=sg)


def check_and_pack(name, case, ref, store):
    o = PO.run(case, torch.float64, grad=True)
    assert len(o["items"]) == len(ref["items"]), (name, len(o["items"]), len(ref["items"]))
    dots, coss, labels = [], [], []
    for (dot, cos, label), want in zip(o["items"], ref["items"]):
        assert dot.shape == want["dot_product"].shape and torch.equal(label, want["label"]), name
        assert float((dot - want["dot_product"]).abs().max()) <= 1e-12 and float((cos - want["cosine_similarity"]).abs().max()) <= 1e-12, name
        dots.append(want["dot_product"].detach().numpy().reshape(-1))
        coss.append(want["cosine_similarity"].detach().numpy().reshape(-1))
        labels.append(want["label"].numpy().reshape(-1))
    items, neg, start = PO.plan_arrays(o["plan"])
    assert all(len(d) == start[n + 1] - start[n] + 1 for n, d in enumerate(dots)), name
    ref_sg = PO.sg_array(case, ref["sg"])
    got_sg = PO.sg_array(case, o["sg"])
    assert np.array_equal(np.isnan(ref_sg), np.isnan(got_sg)) and float(np.nanmax(np.abs(ref_sg - got_sg), initial=0.0)) <= 1e-12, name
    for k, v in zip(("loss_reid", "loss_aux_reid"), o["losses"]):
        assert abs(float(v) - float(ref["raw"][k])) <= 1e-12 and abs(float(o["weighted"][k]) - float(ref["weighted"][k])) <= 1e-12, (name, k)
    assert float((o["embeds"].grad - ref["grad"]).abs().max()) <= 1e-12, name
    o32 = PO.run(case, torch.float32)
    assert o32["plan"] == o["plan"] and all((o32["sim"][k] > 0) == (o["sim"][k] > 0) for k in o["sim"]), name
    negative = [k for k, v in o["sim"].items() if float(v) < 0]
    assert set(negative) == set(case["flip"]), (name, negative)
    margin = PO.min_abs_sim(o["sim"], skip=negative)
    assert margin >= PO.SIM_MARGIN, (name, margin)
    store[f"{name}_items"], store[f"{name}_neg"], store[f"{name}_neg_start"] = items, neg, start
    store[f"{name}_dot"] = np.concatenate(dots) if dots else np.zeros(0)
    store[f"{name}_cos"] = np.concatenate(coss) if coss else np.zeros(0)
    store[f"{name}_label"] = np.concatenate(labels) if labels else np.zeros(0, np.int64)
    store[f"{name}_sg"] = ref_sg
    store[f"{name}_losses"] = np.asarray([float(ref["raw"]["loss_reid"]), float(ref["raw"]["loss_aux_reid"])])
    store[f"{name}_weighted"] = np.asarray([float(ref["weighted"]["loss_reid"]), float(ref["weighted"]["loss_aux_reid"])])
    store[f"{name}_grad"] = ref["grad"].numpy()
    store[f"{name}_checksum"] = PO.checksum(case)
    store[f"{name}_min_abs_sim"] = np.asarray(margin)
    store[f"{name}_counts"] = np.asarray([o["counts"][k] for k in PO.BRANCHES], np.int64)
    return margin, o["counts"]


def main():
    warnings.simplefilter("ignore")
    mod = _load_reference(os.path.abspath(sys.argv[1]))
    store, total = {}, dict.fromkeys(PO.BRANCHES, 0)
    for name, case in list(PO.CASES.items()) + [("e2e", PO.E2E)]:
        ref = reference_run(mod, case)
        margin, counts = check_and_pack(name, case, ref, store)
        for k, v in counts.items():
            total[k] += int(v)
        print(f"{name}: {len(ref['items'])} items, smallest |sim| {margin:.3e}, losses {store[name + '_losses'].tolist()}")
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, f"branches never taken: {missing}"
    print("branches:", total)
    if "--check" in sys.argv:
        print("checked, nothing written")
        return
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
