"""Fixture F26 (tests/golden/f26_seg.npz): the reference's own ``semantic_inference``, ``panoptic_inference`` and ``instance_inference``
(``TimesformerMaskFormer``, downstream/OVIS/mask2former/timesformer_maskformer_model.py) in fp64 on the CPU, over the planted scenario of
tests/seg_oracle.py, at both geometries, both resample orders for the semantic map, and with and without the thing filter for instances.

    python tools/make_golden_seg.py /path/to/reference

The path argument goes on sys.path (never on the GPU machine; nothing of the reference is stored).  detectron2 is not needed: as in
tools/make_golden_vis.py, stand-ins written from the call sites are registered for ``configurable`` (identity), the registry,
``sem_seg_postprocess`` (crop to the image size, bilinear resize), ``Instances`` (an attribute bag made from an image size), ``Boxes`` (holds
its tensor) and ``retry_if_cuda_oom`` (identity); the backbone, criterion and matcher modules the file imports are bare stand-ins, and the
package above it is a namespace module, so that its detectron2-importing ``__init__`` never runs.  The three functions are the reference's
own, called on a stand-in ``self`` that carries ``sem_seg_head.num_classes``, ``num_queries``, the two thresholds, ``metadata``,
``panoptic_on``, ``test_topk_per_image`` and ``device``; what ``forward`` does around them (the upsample to the padded size,
``sem_seg_postprocess`` before or after) is restated here line by line.

Before anything is written the generator checks (and tests/test_seg_cpu.py checks again) that tests/seg_oracle.py agrees with the
reference exactly on every discrete output and to 1e-12 on every float, that every score-threshold and overlap-ratio decision and every
top-k gap has a relative margin of at least 1e-3, that every overlap decision keeps its side when each area moves by the number of
undecided pixels, and that the oracle in fp32 gives the same discrete outputs as in fp64.  Stored: the inputs as fp16 (exact); per case
and geometry the panoptic map (int8), segments_info, the query-to-segment table and the three counts per query; per geometry the
instance labels, rows, scores (fp64) and bit-packed masks, with and without the thing filter, and the semantic maps of both orders
(fp64, every STRIDE-th row and column: they pin the oracle, which gives the tests the whole map).  Every array is a pure function of the
seed: a second run writes the same bytes.
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
from tests import seg_oracle as SO      # noqa: E402

PKG = ("downstream", "OVIS", "mask2former")
STRIDE = {"down": 2, "up": 3}


def _module(name, package=False, path=None, **attrs):
    m = types.ModuleType(name)
    if package:
        m.__path__ = [path] if path else []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class _Registry:
    def register(self, obj=None):
        return obj if obj is not None else (lambda o: o)


class Instances:
    def __init__(self, image_size):
        self.image_size = tuple(image_size)


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


def sem_seg_postprocess(result, img_size, output_height, output_width):
    result = result[:, :img_size[0], :img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


def _load_reference(ref_root):
    ident = lambda f=None, **k: f if f is not None else (lambda g: g)      # noqa: E731
    _module("detectron2", package=True)
    _module("detectron2.config", configurable=ident)
    _module("detectron2.data", MetadataCatalog=None)
    _module("detectron2.modeling", package=True, META_ARCH_REGISTRY=_Registry(), ShapeSpec=None, build_backbone=None, build_sem_seg_head=None)
    _module("detectron2.modeling.backbone", Backbone=object)
    _module("detectron2.modeling.postprocessing", sem_seg_postprocess=sem_seg_postprocess)
    _module("detectron2.structures", BitMasks=object, Boxes=Boxes, ImageList=object, Instances=Instances)
    _module("detectron2.utils", package=True)
    _module("detectron2.utils.memory", retry_if_cuda_oom=lambda f: f)
    _module("models", package=True)
    _module("models.modeling_timesformer_siglip_adapter", TimesformerMultiTaskingModelSigLIPViTAdapter=object)
    for i in range(len(PKG)):
        _module(".".join(PKG[:i + 1]), package=True, path=os.path.join(ref_root, *PKG[:i + 1]))
    name = ".".join(PKG)
    _module(name + ".modeling", package=True)
    _module(name + ".modeling.criterion", SetCriterion=object)
    _module(name + ".modeling.matcher", HungarianMatcher=object)
    sys.path.insert(0, ref_root)
    return importlib.import_module(name + ".timesformer_maskformer_model").TimesformerMaskFormer


def stand_in(kw, panoptic_on):
    things = {100 + c: c for c in kw["thing_classes"]}
    return types.SimpleNamespace(sem_seg_head=types.SimpleNamespace(num_classes=kw["num_classes"]), num_queries=SO.QUERIES,
                                 object_mask_threshold=kw["object_mask_threshold"], overlap_threshold=kw["overlap_threshold"],
                                 metadata=types.SimpleNamespace(thing_dataset_id_to_contiguous_id=things), panoptic_on=panoptic_on,
                                 test_topk_per_image=SO.TOPK, device=torch.device("cpu"))


def main():
    warnings.simplefilter("ignore")
    ref = _load_reference(os.path.abspath(sys.argv[1]))
    cls32, masks32 = SO.make_scenario()
    cls, masks = cls32.double(), masks32.double()
    out = {"mask_cls": cls32.numpy().astype(np.float16), "mask_pred": masks32.numpy().astype(np.float16)}
    smallest = (None, np.inf)

    def note(where, margins):
        nonlocal smallest
        for what, m in margins:
            if m < smallest[1]:
                smallest = (f"{where}: {what}", m)

    for gname, g in SO.GEOMETRIES.items():
        padded = F.interpolate(masks[None], size=tuple(g["padded"]), mode="bilinear", align_corners=False)[0]      # forward: upsample masks
        post = sem_seg_postprocess(padded, g["crop"], *g["out"])
        # semantic, both orders
        me = stand_in(SO.CASES["planted"], False)
        before = ref.semantic_inference(me, cls, post)
        after = sem_seg_postprocess(ref.semantic_inference(me, cls, padded), g["crop"], *g["out"])
        for name, want, flag in (("before", before, True), ("after", after, False)):
            mine = SO.semantic(cls32, masks32, g, before=flag)
            assert float((mine - want).abs().max()) <= 1e-12, (gname, name)
            out[f"{gname}.sem_{name}"] = want.numpy()[:, ::STRIDE[gname], ::STRIDE[gname]].copy()
        assert float((before - after).abs().max()) > 1e-3, "the two resample orders are indistinguishable"
        # panoptic
        for case, kw in SO.CASES.items():
            pan, info = ref.panoptic_inference(stand_in(kw, True), cls, post)
            mine = SO.panoptic(cls32, masks32, g, kw)
            mine32 = SO.panoptic(cls32, masks32, g, kw, dtype=torch.float32)
            assert pan.dtype == torch.int32 and torch.equal(pan, mine["map"]) and info == mine["segments_info"], (gname, case)
            assert torch.equal(mine32["map"], mine["map"]) and mine32["segments_info"] == info and np.array_equal(mine32["counts"], mine["counts"]), \
                (gname, case, "fp32 decides otherwise")
            note(f"{gname}.{case}", mine["margins"])
            slack = int(SO.undecided(mine, *SO.bands(mine, mine32)).sum())
            assert SO.overlap_decisions_hold(mine, kw, slack), (gname, case, slack)
            print(f"{gname}.{case}: segments {info}, query -> segment {mine['segment_of_query']}, undecided pixels {slack} of {pan.numel()}")
            print("   counts (won, r >= 0, both):", mine["counts"].tolist())
            assert int(pan.max()) < 128
            out.update({f"{gname}.{case}.map": pan.numpy().astype(np.int8), f"{gname}.{case}.info": SO.info_array(info),
                        f"{gname}.{case}.segment_of_query": np.array(mine["segment_of_query"], np.int32), f"{gname}.{case}.counts": mine["counts"].astype(np.int32)})
        # instances, without and with the thing filter
        for name, things in (("inst", None), ("inst_things", SO.THINGS)):
            r = ref.instance_inference(stand_in(SO.CASES["planted"], things is not None), cls, post)
            mine = SO.instance(cls32, masks32, g, things=things)
            mine32 = SO.instance(cls32, masks32, g, things=things, dtype=torch.float32)
            # the reference's topk is unsorted: bring its instances into the oracle's order by (query row, label), which is unique
            key = lambda rows, labels: [(int(a), int(b)) for a, b in zip(rows, labels)]      # noqa: E731
            ref_rows = [next(q for q in range(SO.QUERIES) if torch.equal(m > 0.5, post[q] > 0)) for m in r.pred_masks]
            ref_key = key(ref_rows, r.pred_classes)
            perm = [ref_key.index(k) for k in key(mine["rows"], mine["labels"])]
            assert sorted(perm) == list(range(len(ref_key))), (gname, name)
            assert r.image_size == tuple(g["out"]) and r.pred_boxes.tensor.shape == (len(perm), 4) and not r.pred_boxes.tensor.any()
            assert float((r.scores[perm] - mine["scores"]).abs().max()) <= 1e-12, (gname, name)
            assert torch.equal(r.pred_masks[perm] > 0.5, mine["masks"]) and r.pred_masks.dtype == torch.float32
            assert torch.equal(mine32["labels"], mine["labels"]) and torch.equal(mine32["rows"], mine["rows"]), "fp32 picks otherwise"
            note(f"{gname}.{name}", mine["margins"])
            print(f"{gname}.{name}: rows {mine['rows'].tolist()}, labels {mine['labels'].tolist()}")
            out.update({f"{gname}.{name}.scores": mine["scores"].numpy(), f"{gname}.{name}.labels": mine["labels"].numpy().astype(np.int32),
                        f"{gname}.{name}.rows": mine["rows"].numpy().astype(np.int32), f"{gname}.{name}.masks": SO.pack_bits(mine["masks"].flatten(1).numpy())})
    print(f"smallest decision margin {smallest[1]:.3e} ({smallest[0]})")
    assert smallest[1] >= SO.MIN_MARGIN, "a decision of the scenario is too close for fp32: change the seed or the planted scores"
    os.makedirs(os.path.dirname(SO.GOLDEN), exist_ok=True)
    np.savez_compressed(SO.GOLDEN, **out)
    print(SO.GOLDEN, os.path.getsize(SO.GOLDEN), "bytes")
    assert os.path.getsize(SO.GOLDEN) <= 256 << 10, "F26 has left the size class of F25"


if __name__ == "__main__":
    main()
