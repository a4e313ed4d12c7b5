"""Fixture F25 (tests/golden/f25_vis.npz): the reference's own ``SimpleTracker`` (with ``MemoryBank``, ``Tracklet`` and ``mask_nms``) and
``CTVISModel.inference_video`` in fp64 on the CPU, over the synthetic scenario of tests/vis_oracle.py.

    python tools/make_golden_vis.py /path/to/reference

The path argument goes on sys.path (never on the GPU machine; nothing of the reference is stored).  detectron2, fvcore and torchvision
are not needed: as in tools/make_golden_mask_decoder.py, stand-ins written from the call sites are registered for
``detectron2.config.configurable`` (identity), the registries, ``detectron2.structures`` and ``torchvision.ops.boxes.box_area``, and the
packages above the modules that are loaded are bare namespace modules pointing at the reference's directories, so that their
detectron2-importing ``__init__`` files never run (the names those ``__init__`` files would re-export are set by hand).

The reference hard-codes the GPU: ``Tracklet.__init__`` makes ``torch.zeros(..., device='cuda')`` and ``SimpleTracker.device`` returns
``torch.device('cuda')``.  The generator runs without one, so the two reference modules (``memory_bank``, ``simple_tracker``) get a
module-level ``torch`` PROXY that forwards every attribute to torch and maps a ``cuda`` device argument of ``zeros`` / ``device`` to the
CPU, and the ``device`` property is patched to the CPU.  No arithmetic is touched.  ``inference_video`` is the reference's own function
called on a stand-in ``self`` that carries ``num_topk``, the two chunk sizes, ``device`` and ``sem_seg_head.num_classes``.

What the reference does not return is recovered from what it does: the query indices that survive the selection and the NMS by wrapping
``mask_nms`` and ``track`` and matching their mask / embedding rows to the frame's (they are unique), the index table by matching the
returned masks to the detections' rows, the instance ids from the two.

Before anything is written the generator checks (and tests/test_vis_cpu.py checks again) that tests/vis_oracle.py agrees with the
reference exactly on every discrete output and to 1e-12 on every float, and that the smallest recorded decision margin is at least
1e-3, and that no alternative is indistinguishable from the default in what the tests compare (ids and index table for hungarian, the
match-score matrices for cosine, the memory bank's embeddings for the embed types, the final logits for max).  Stored per case of
vis_oracle.CASES: selections, kept sets, ids, instance table, index table, final logits (fp64), the memory bank's ids and embeddings in
every frame (recorded from the reference's ``MemoryBank.exist_reid_embeds``); per case and geometry: scores, labels, rows, numerator,
denominator (fp64 / ints) and the bit-packed output masks.  The inputs are stored
once, as fp16 (exact).  Every array is a pure function of the seed: a second run writes the same bytes.
"""
import importlib
import importlib.machinery
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vis_oracle as VO      # noqa: E402

CTVIS = ("downstream", "OVIS", "ctvis")


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
    def __init__(self, *a):
        pass

    def register(self, obj=None):
        return obj if obj is not None else (lambda o: o)


class _TorchProxy:
    """torch, with the ``cuda`` device mapped to the CPU where the reference names it."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def zeros(*args, device=None, **kw):
        return torch.zeros(*args, device="cpu" if str(device).startswith("cuda") else device, **kw)

    @staticmethod
    def device(*args):
        return torch.device("cpu") if args and str(args[0]).startswith("cuda") else torch.device(*args)


def _load_reference(ref_root):
    ident = lambda f=None, **k: f if f is not None else (lambda g: g)      # noqa: E731
    _module("detectron2", package=True)
    _module("detectron2.config", configurable=ident)
    _module("detectron2.utils", package=True)
    _module("detectron2.utils.registry", Registry=_Registry)
    _module("detectron2.modeling", META_ARCH_REGISTRY=_Registry())
    _module("detectron2.structures", BitMasks=object, ImageList=object)
    _module("torchvision", package=True)
    _module("torchvision.ops", package=True)
    _module("torchvision.ops.boxes", box_area=lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    base = os.path.join(ref_root, *CTVIS)
    for i in range(len(CTVIS)):
        _module(".".join(CTVIS[:i + 1]), package=True, path=os.path.join(ref_root, *CTVIS[:i + 1]))
    name = ".".join(CTVIS)
    _module(name + ".utils", package=True, path=os.path.join(base, "utils"))
    _module(name + ".modeling", package=True, path=os.path.join(base, "modeling"))
    _module(name + ".modeling.tracker", package=True, path=os.path.join(base, "modeling", "tracker"), build_tracker=None)
    _module(name + ".modeling.cl_plugin", build_cl_plugin=None)
    _module(".".join(CTVIS[:2]) + ".mask2former", MaskFormer=torch.nn.Module, TimesformerMaskFormer=torch.nn.Module)
    sys.path.insert(0, ref_root)
    utils = importlib.import_module(name + ".utils.utils")
    memory = importlib.import_module(name + ".utils.memory")
    sys.modules[name + ".utils"].mask_nms = utils.mask_nms
    sys.modules[name + ".utils"].retry_if_cuda_oom = memory.retry_if_cuda_oom
    bank = importlib.import_module(name + ".modeling.tracker.memory_bank")
    tracker = importlib.import_module(name + ".modeling.tracker.simple_tracker")
    bank.torch = tracker.torch = _TorchProxy()
    tracker.SimpleTracker.device = property(lambda self: torch.device("cpu"))
    model = importlib.import_module(name + ".ctvis_model")
    return tracker, model


def _row_of(table, row):
    hits = [i for i in range(table.shape[0]) if torch.equal(table[i], row)]
    assert len(hits) == 1, hits
    return hits[0]


def run_reference_tracker(tracker_mod, det, kw):
    trk = tracker_mod.SimpleTracker(**kw)
    selected, kept, ids, frame, bank = [], [], [], [0], {}
    nms, track = tracker_mod.mask_nms, trk.track
    exist = tracker_mod.MemoryBank.exist_reid_embeds

    def exist_recording(self, frame_id):
        r = exist(self, frame_id)
        bank[frame_id] = ([int(i) for i in r[0]], r[1].clone())
        return r

    def nms_recording(seg_masks, scores, nms_thr=0.5):
        selected.append([_row_of(det["pred_masks"][frame[0]], m[0]) for m in seg_masks])
        return nms(seg_masks, scores, nms_thr=nms_thr)

    def track_recording(pred_scores, pred_logits, pred_masks, pred_embeds, pred_queries, frame_id):
        kept.append([_row_of(det["pred_embeds"][frame_id], e) for e in pred_embeds])
        r = track(pred_scores, pred_logits, pred_masks, pred_embeds, pred_queries, frame_id)
        ids.append([int(i) for i in r[0]])
        frame[0] = frame_id + 1
        return r

    tracker_mod.mask_nms, trk.track, tracker_mod.MemoryBank.exist_reid_embeds = nms_recording, track_recording, exist_recording
    try:
        out = trk.inference(det, None)
    finally:
        tracker_mod.mask_nms, tracker_mod.MemoryBank.exist_reid_embeds = nms, exist
    return out, selected, kept, ids, bank


def pad_bank(embeds, frames, width):
    """Per-frame [n_f, E] tensors (or None) as one zero-padded [F, n_max, E] array."""
    n = max([e.shape[0] for e in embeds if e is not None] + [1])
    out = np.zeros((frames, n, width), np.float64)
    for f, e in enumerate(embeds):
        if e is not None:
            out[f, :e.shape[0]] = e.numpy()
    return out


def main():
    warnings.simplefilter("ignore")
    tracker_mod, model_mod = _load_reference(os.path.abspath(sys.argv[1]))
    det32 = VO.make_scenario()
    det = {k: v.double() for k, v in det32.items()}
    Fr, Q = det["pred_logits"].shape[:2]
    flat_masks = det["pred_masks"].flatten(0, 1)
    out = {k: v.numpy().astype(np.float16) for k, v in det32.items()}
    smallest, tracked = (None, np.inf), {}
    for case in VO.CASES:
        kw = VO.tracker_kwargs(case)
        ref, selected, kept, ids, bank = run_reference_tracker(tracker_mod, det, kw)
        mine = VO.track(det, kw)
        for f in range(Fr):                                   # the memory bank the reference matched against, frame by frame
            want_ids, want_emb = bank.get(f, ([], None))
            assert mine["bank_ids"][f] == want_ids, (case, f)
            assert (want_emb is None) == (mine["bank_embeds"][f] is None), (case, f)
            if want_emb is not None:
                assert float((want_emb - mine["bank_embeds"][f]).abs().max()) <= 1e-12, (case, f)
        assert selected == mine["selected"] and kept == mine["kept"] and ids == mine["ids"], case
        logits, masks = ref["pred_logits"][0], ref["pred_masks"][0]
        K = masks.shape[0]
        index = np.full((K, Fr), -1, np.int32)
        for k in range(K):
            for f in range(Fr):
                if masks[k, f].any():
                    index[k, f] = f * Q + _row_of(det["pred_masks"][f], masks[k, f])
        instances = []
        for k in range(K):
            seen = {ids[f][mine["tracked"][f].index(int(index[k, f]) - f * Q)] for f in range(Fr) if index[k, f] >= 0}
            assert len(seen) == 1, (case, k, seen)
            instances.append(seen.pop())
        assert np.array_equal(index, mine["index"]) and instances == mine["instances"], case
        assert float((logits - mine["logits"]).abs().max()) <= 1e-12, case
        assert torch.equal(masks, VO.dense_masks(det, index)), case
        worst = min(mine["margins"], key=lambda m: m[1])
        smallest = min(smallest, (f"{case}: {worst[0]}", worst[1]), key=lambda m: m[1])
        out.update({f"{case}.selected": VO.ragged(selected), f"{case}.kept": VO.ragged(kept), f"{case}.ids": VO.ragged(ids),
                    f"{case}.instances": np.array(instances, np.int32), f"{case}.index": index, f"{case}.logits": logits.numpy(),
                    f"{case}.bank_ids": VO.ragged(mine["bank_ids"]), f"{case}.bank_embeds": pad_bank([bank.get(f, (0, None))[1] for f in range(Fr)], Fr, VO.EMBED)})
        tracked[case] = mine
        print(f"{case}: {K} instances {instances}, smallest margin {worst[1]:.3e} ({worst[0]}), rules: "
              f"nms removed {sum(len(s) - len(k) for s, k in zip(selected, kept))}, absent entries {int((index < 0).sum())}")
        if True:
            stand_in = types.SimpleNamespace(num_topk=VO.NUM_TOPK, test_interpolate_chunk_size=5, test_instance_chunk_size=5, device=torch.device("cpu"),
                                             sem_seg_head=types.SimpleNamespace(num_classes=VO.CLASSES))
            for gname, g in VO.GEOMETRIES.items():
                video = model_mod.CTVISModel.inference_video(stand_in, ref["pred_logits"].clone(), ref["pred_masks"], (Fr, 3) + tuple(g["padded"]), g["crop"],
                                                             g["out"][0], g["out"][1], "cpu")
                got = VO.inference_video(mine["logits"], VO.dense_masks(det, index), g)
                assert video["pred_labels"] == got["labels"].tolist() and video["image_size"] == tuple(g["out"]), gname
                assert max(abs(a - b) for a, b in zip(video["pred_scores"], got["scores"].tolist())) <= 1e-12, gname
                assert all(torch.equal(a, b) for a, b in zip(video["pred_masks"], got["masks"])), gname
                worst = min(got["margins"], key=lambda m: m[1])
                smallest = min(smallest, (f"{case} {gname}: topk", worst[1]), key=lambda m: m[1])
                band = 4 * 2.0 ** -24 * float(got["logits"].abs().max())
                present = torch.from_numpy(index >= 0)[got["rows"]][:, :, None, None].expand_as(got["logits"])
                print(f"  {gname}: labels {video['pred_labels']}, share of present pixels with |logit| <= {band:.2e}: "
                      f"{float((got['logits'][present].abs() <= band).double().mean()):.5f}")
                gname = f"{case}.{gname}"
                out.update({f"{gname}.scores": np.array(video["pred_scores"], np.float64), f"{gname}.labels": np.array(video["pred_labels"], np.int32),
                            f"{gname}.rows": got["rows"].numpy().astype(np.int32), f"{gname}.numerator": got["numerator"].numpy(),
                            f"{gname}.denominator": got["denominator"].numpy().astype(np.int64),
                            f"{gname}.masks": VO.pack_bits(torch.stack(video["pred_masks"]).flatten(1).numpy())})
    # no alternative may pass by being indistinguishable from the default in what the tests compare
    d = tracked["default"]
    differs = lambda a, b: any((x is None) != (y is None) or (x is not None and (x.shape != y.shape or float((x - y).abs().max()) > 1e-3))      # noqa: E731
                               for x, y in zip(a, b))
    assert tracked["hungarian"]["ids"] != d["ids"] and not np.array_equal(tracked["hungarian"]["index"], d["index"]), "hungarian == greedy"
    assert differs(tracked["cosine"]["match"], d["match"]), "cosine == bisoftmax"
    for case in ("last", "weighted", "momentum"):
        assert differs(tracked[case]["bank_embeds"], d["bank_embeds"]), f"{case} == similarity_guided"
        for other in ("last", "weighted", "momentum"):
            assert other == case or differs(tracked[case]["bank_embeds"], tracked[other]["bank_embeds"]), (case, other)
    assert float((tracked["max"]["logits"] - d["logits"]).abs().max()) > 1e-3, "max == mean"
    print(f"smallest decision margin {smallest[1]:.3e} ({smallest[0]})")
    assert smallest[1] >= VO.MIN_MARGIN, "a decision of the scenario is too close for fp32: change the seed or the planted scores"
    os.makedirs(os.path.dirname(VO.GOLDEN), exist_ok=True)
    np.savez_compressed(VO.GOLDEN, **out)
    print(VO.GOLDEN, os.path.getsize(VO.GOLDEN), "bytes")
    assert os.path.getsize(VO.GOLDEN) <= 1 << 20, "a fixture file above 1 MiB"


if __name__ == "__main__":
    main()
