"""Image segmentation after the mask decoder on the MI355X: the native semantic, panoptic and instance inference against the reference's
operator sequence in torch on the same GPU, in the same process.

    python tools/seg_bench.py            # the shipped COCO shape: Q = 100, C = 80 (80 things), top-k 100, masks 200 x 304, padded and
                                         # output 800 x 1216, and C = 133 (80 things) for semantic / panoptic -> profiles/seg.txt
    python tools/seg_bench.py --smoke    # a tiny shape, two runs, no file

composed: ``F.interpolate`` of the [Q, h, w] masks to the padded size, ``sem_seg_postprocess`` (crop, ``F.interpolate``), then the
reference's ``semantic_inference`` (softmax, sigmoid, einsum), ``panoptic_inference`` (its Python loop with four ``.item()`` per kept
query) and ``instance_inference``, restated here on GPU tensors; every read-back is counted.  The resample is part of every composed
mode, as it is part of every native one.  The panoptic paths end on the host (the native one in its one copy, the composed one in its
read-backs), so all modes are timed with a host clock around a call that starts and ends synchronised; medians of 10 runs after warm-up.
A row where the native path loses is reported as it is.
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
from streamformer_amd import segmentation as seg   # noqa: E402

SHIPPED = [dict(Q=100, C=80, things=80, src=(200, 304), padded=(800, 1216), crop=(800, 1216), out=(800, 1216), topk=100, modes=("semantic", "panoptic", "instance")),
           dict(Q=100, C=133, things=80, src=(200, 304), padded=(800, 1216), crop=(800, 1216), out=(800, 1216), topk=100, modes=("semantic", "panoptic"))]
SMOKE = [dict(Q=12, C=5, things=3, src=(12, 20), padded=(48, 80), crop=(45, 77), out=(75, 130), topk=6, modes=("semantic", "panoptic", "instance"))]
THRESHOLDS = dict(object_mask_threshold=0.8, overlap_threshold=0.8)


def make_image(s, dev):
    """Seeded decoder outputs: 30 confident queries with box masks (some overlapping) among no-object queries."""
    g = torch.Generator().manual_seed(26)
    Q, C, (h, w) = s["Q"], s["C"], s["src"]
    logits = torch.randn(Q, C + 1, generator=g) - 2.0
    logits[:, C] += 6.0
    masks = torch.randn(Q, h, w, generator=g) * 2 - 10
    for k in range(min(30, Q)):
        y, x = (k * 37) % (h - h // 3), (k * 53) % (w - w // 3)
        logits[k, (k * 7) % C] += 10.0
        logits[k, C] -= 6.0
        masks[k, y:y + h // 3, x:x + w // 3] += 20
    return logits.to(dev), masks.to(dev)


def composed_resample(masks, s):
    m = F.interpolate(masks[None], size=s["padded"], mode="bilinear", align_corners=False)[0]
    return F.interpolate(m[:, :s["crop"][0], :s["crop"][1]][None], size=s["out"], mode="bilinear", align_corners=False)[0]


def composed_semantic(cls, masks, s, syncs):
    return torch.einsum("qc,qhw->chw", F.softmax(cls, dim=-1)[..., :-1], composed_resample(masks, s).sigmoid())


def composed_panoptic(cls, masks, s, syncs):
    item = lambda v: (syncs.append(1), v.item())[1]      # noqa: E731
    mask_pred = composed_resample(masks, s)
    scores, labels = F.softmax(cls, dim=-1).max(-1)
    mask_pred = mask_pred.sigmoid()
    keep = labels.ne(s["C"]) & (scores > THRESHOLDS["object_mask_threshold"])
    cur_scores, cur_classes, cur_masks = scores[keep], labels[keep], mask_pred[keep]      # boolean indexing: one synchronisation each
    syncs.extend([1, 1, 1])
    cur_prob_masks = cur_scores.view(-1, 1, 1) * cur_masks
    panoptic_seg = torch.zeros(cur_masks.shape[-2:], dtype=torch.int32, device=cur_masks.device)
    segments_info, current, stuff = [], 0, {}
    if cur_masks.shape[0] == 0:
        return panoptic_seg, segments_info
    ids = cur_prob_masks.argmax(0)
    for k in range(cur_classes.shape[0]):
        pred_class = item(cur_classes[k])
        isthing = pred_class < s["things"]
        mask_area = item((ids == k).sum())
        original_area = item((cur_masks[k] >= 0.5).sum())
        mask = (ids == k) & (cur_masks[k] >= 0.5)
        if mask_area > 0 and original_area > 0 and item(mask.sum()) > 0:
            if mask_area / original_area < THRESHOLDS["overlap_threshold"]:
                continue
            if not isthing:
                if pred_class in stuff:
                    panoptic_seg[mask] = stuff[pred_class]
                    continue
                stuff[pred_class] = current + 1
            current += 1
            panoptic_seg[mask] = current
            segments_info.append({"id": current, "isthing": bool(isthing), "category_id": pred_class})
    return panoptic_seg, segments_info


def composed_instance(cls, masks, s, syncs):
    mask_pred = composed_resample(masks, s)
    scores = F.softmax(cls, dim=-1)[:, :-1]
    top_scores, top = scores.flatten(0, 1).topk(s["topk"], sorted=False)
    labels = top % s["C"]
    mask_pred = mask_pred[top // s["C"]]
    pred_masks = (mask_pred > 0).float()
    mask_scores = (mask_pred.sigmoid().flatten(1) * pred_masks.flatten(1)).sum(1) / (pred_masks.flatten(1).sum(1) + 1e-6)
    return pred_masks, top_scores * mask_scores, labels


def host_timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoke", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X: there is nothing to time on a CPU"
    dev = torch.device("cuda:0")
    runs, warmup = (2, 1) if args.smoke else (10, 3)
    lines = []
    for s in (SMOKE if args.smoke else SHIPPED):
        cls, masks = make_image(s, dev)
        geo = dict(padded=s["padded"], crop=s["crop"], out=s["out"])
        things = range(s["things"])
        lines.append(f"shape: Q {s['Q']}, classes {s['C']} ({s['things']} things), masks {s['src']}, padded {s['padded']}, crop {s['crop']}, output {s['out']}, "
                     f"top-k {s['topk']}; host clock, median (min, max) ms of {runs}")
        native = {"semantic": lambda: sa.semantic_inference(cls, masks, geo),
                  "panoptic": lambda: sa.panoptic_inference(cls, masks, geo, num_classes=s["C"], thing_classes=things, **THRESHOLDS),
                  "instance": lambda: sa.instance_inference(cls, masks, geo, num_classes=s["C"], test_topk_per_image=s["topk"])}
        composed = {"semantic": composed_semantic, "panoptic": composed_panoptic, "instance": composed_instance}
        for mode in s["modes"]:
            copies, real = [], seg._device_to_host
            seg._device_to_host = lambda t: (copies.append(1), real(t))[1]
            a = native[mode]()
            seg._device_to_host = real
            syncs = []
            b = composed[mode](cls, masks, s, syncs)
            if mode == "semantic":
                agree = f"largest difference {float((a - b).abs().max()):.2e}"
            elif mode == "panoptic":
                agree = f"segments {len(a[1])} vs {len(b[1])}, segments_info equal: {a[1] == b[1]}, pixels differing {int((a[0] != b[0]).sum())} of {a[0].numel()}"
            else:
                order = torch.argsort(b[1], descending=True, stable=True)
                mine = torch.argsort(a.scores, descending=True, stable=True)
                agree = (f"{len(a)} instances, largest score difference {float((a.scores[mine] - b[1][order]).abs().max()):.2e}, mask pixels differing "
                         f"{int((a.pred_masks[mine] != b[0][order]).sum())}")
            nat_t = host_timed(native[mode], warmup, runs)
            ref_t = host_timed(lambda: composed[mode](cls, masks, s, []), warmup, runs)
            extra = ""
            if mode == "semantic":
                out_bytes = s["C"] * s["out"][0] * s["out"][1] * 4
                extra = f", {out_bytes / nat_t[0] / 1e6:.1f} GB/s of the {out_bytes / 1e6:.0f} MB output stream"
            lines.append(f"  {mode}: native {nat_t[0]:.3f} ({nat_t[1]:.3f}, {nat_t[2]:.3f}) with {len(copies)} host synchronisation(s){extra}; composed {ref_t[0]:.3f} "
                         f"({ref_t[1]:.3f}, {ref_t[2]:.3f}) with {len(syncs)} host synchronisation(s); composed / native {ref_t[0] / nat_t[0]:.2f}; {agree}")
    print("\n".join(lines))
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "seg.txt")
        if not os.path.exists(path):                         # the first hardware run is the record; later runs print only
            with open(path, "w") as fh:
                fh.write("tools/seg_bench.py on an MI355X\n" + "\n".join(lines) + "\n")
            print("wrote", path)


if __name__ == "__main__":
    main()
