"""Video instance segmentation after the mask decoder on the MI355X: the native tracker front + host loop and the native mask
post-processing against the reference's operator sequences in torch on the same GPU.

    python tools/vis_bench.py            # the shipped YouTube-VIS shape: Q = 100, a 36-frame video, masks 120 x 214, padded 480 x 864,
                                         # crop 480 x 853, output 720 x 1280, top-k 10, 40 classes, E = 256 -> profiles/vis.txt
    python tools/vis_bench.py --smoke    # a tiny shape, two runs, no file

(i)  tracker.  native: ``SimpleTracker.inference(det, dense_masks=False)`` (three launches, ONE device-to-host copy, the loop on the host).
     composed: the reference's sequence restated here on GPU tensors: per frame softmax / max / sort / threshold, ``mask_nms`` with its
     per-pair ``iou > thr`` read-back, ``torch.mm`` + the two softmaxes, the greedy loop with ``torch.max`` and a read-back per instance,
     the momentum and similarity-guided updates, one ``.item()`` per tracked instance.  Every read-back of the composed path is counted.
     Both end on the host (the native path in its one copy, the composed one in its read-backs), so HIP events would miss the time the
     host spends between launches: part (i) is timed with a host clock around a call that starts and ends synchronised
     (``host_timed`` below), not with tools/_timing.py's event pairs.
(ii) post-processing.  native: ``sf_op_vis_postprocess`` through ``vis.resample_masks`` (bool masks + numerator + denominator).
     composed: ``inference_video``'s two ``F.interpolate`` calls with the crop, the threshold and the sigmoid sums, in the reference's
     chunks of five instances x five frames.  HIP events (tools/_timing.py).
Medians of 10 runs after warm-up.  A row where the native path loses is reported as it is.
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
from streamformer_amd import vis   # noqa: E402
from tools._timing import timed    # noqa: E402

SHIPPED = dict(F=36, Q=100, C=40, E=256, src=(120, 214), padded=(480, 864), crop=(480, 853), out=(720, 1280), topk=10, objects=12)
SMOKE = dict(F=4, Q=8, C=5, E=32, src=(23, 37), padded=(92, 148), crop=(90, 145), out=(67, 111), topk=3, objects=3)


def make_clip(s, dev):
    """A seeded clip with ``objects`` persistent instances (confident logits, box masks, one embedding each) among background queries."""
    g = torch.Generator().manual_seed(36)
    Fr, Q, C, E, (h, w), n = s["F"], s["Q"], s["C"], s["E"], s["src"], s["objects"]
    logits = torch.randn(Fr, Q, C + 1, generator=g) - 2.0
    logits[..., C] += 6.0
    masks = torch.randn(Fr, Q, h, w, generator=g) * 2 - 10
    embeds = torch.randn(Fr, Q, E, generator=g) * 0.1
    base = torch.randn(n, E, generator=g)
    for k in range(n):
        y, x = (k * 7) % (h - 8), (k * 13) % (w - 12)
        for f in range(Fr):
            logits[f, k, k % C] += 8.0
            logits[f, k, C] -= 6.0
            masks[f, k, y:y + 8, min(x + f, w - 12):min(x + f, w - 12) + 12] += 20
            embeds[f, k] += base[k]
    det = {"pred_logits": logits, "pred_masks": masks, "pred_embeds": embeds, "pred_queries": torch.randn(Fr, Q, E, generator=g)}
    return {k: v.to(dev) for k, v in det.items()}


def composed_tracker(det, kw, syncs):
    """The reference's SimpleTracker.inference (defaults: bisoftmax, greedy, frame_weight, similarity_guided, mean) on GPU tensors."""
    sync = lambda v: (syncs.append(1), v.item())[1]      # noqa: E731
    bank, video, num = {}, {}, 0
    Fr = det["pred_logits"].shape[0]
    for f in range(Fr):
        lg, mk, em = det["pred_logits"][f], det["pred_masks"][f], det["pred_embeds"][f]
        mx = F.softmax(lg, dim=-1)[:, :-1].max(1)[0]
        sc, order = torch.sort(mx, descending=True)
        valid = sc > kw["inference_select_thr"]
        if sync(valid.sum()) == 0:
            valid[0] = True
        sc, lg, mk, em = sc[valid], lg[order][valid], mk[order][valid], em[order][valid]
        seg = (mk.sigmoid() > 0.5).flatten(1).char()
        keep = [True] * len(sc)
        for i in range(len(sc) - 1):
            if keep[i]:
                for j in range(i + 1, len(sc)):
                    if keep[j]:
                        inter = (seg[i] * seg[j]).sum()
                        union = (seg[i] + seg[j] - seg[i] * seg[j]).sum()
                        if sync((inter + 1e-6) / (union + 1e-6) > kw["mask_nms_thr"]):
                            keep[j] = False
        keep = torch.tensor(keep, device=sc.device)
        sc, lg, mk, em = sc[keep], lg[keep], mk[keep], em[keep]
        ids = torch.full((len(sc),), -1, dtype=torch.long, device=sc.device)
        if num > 0 and bank:
            exist_ids = list(bank)
            exist = torch.stack([t["guided"] for t in bank.values()])
            frames = torch.tensor([t["n"] for t in bank.values()], device=sc.device)
            sim = torch.mm(em, exist.t())
            match = (sim.softmax(1) + sim.softmax(0)) / 2
            for i in range(len(sc)):
                above = match[i] > kw["match_score_thr"]
                row = match[i]
                if sync(above.sum()) > 1:
                    wt = frames[above].to(row)
                    row = torch.where(above, row * frames.to(row), row * wt.mean())
                best, col = torch.max(row, dim=0)
                if sync(best > kw["match_score_thr"]):
                    ids[i] = exist_ids[sync(col)]
                    match[:i, col] = 0
                    match[i + 1:, col] = 0
        new = (ids == -1) & (sc > kw["init_score_thr"])
        count = sync(new.sum())
        ids[new] = torch.arange(num, num + count, device=sc.device)
        num += count
        ok = ids > -1
        ids, sc, lg, mk, em = ids[ok], sc[ok], lg[ok], mk[ok], em[ok]
        for k in range(len(ids)):
            inst = sync(ids[k])
            t = bank.setdefault(inst, {"embeds": [], "n": 0, "last": f, "guided": None})
            t["embeds"].append(em[k])
            if t["n"] == 0:
                t["guided"] = em[k]
            else:
                earlier = torch.stack(t["embeds"][:-1])
                s = torch.sum(torch.einsum("bc,c->b", F.normalize(earlier, dim=-1), F.normalize(em[k], dim=-1))) / (len(t["embeds"]) - 1)
                beta = max(0, s)                             # the reference's read-back
                syncs.append(1)
                t["guided"] = (1 - beta) * t["guided"] + beta * em[k]
            t["n"], t["last"] = t["n"] + 1, f
            if len(t["embeds"]) > kw["maximum_cache"]:
                t["embeds"].pop(0)
            v = video.setdefault(inst, {"masks": [None] * f, "logits": [None] * f})
            v["masks"].append(mk[k])
            v["logits"].append(lg[k])
        for dead in [i for i, t in bank.items() if f - t["last"] > kw["num_dead_frames"]]:
            del bank[dead]
        for v in video.values():
            if len(v["masks"]) < f + 1:
                v["masks"].append(None)
                v["logits"].append(None)
        if f > kw["noise_frame_num"]:
            for inst in list(video):
                ms = video[inst]["masks"]
                trailing = next((n for n, m in enumerate(reversed(ms)) if m is not None), len(ms))
                if trailing >= kw["none_frame_num"] and sum(m is not None for m in ms) < kw["suppress_frame_num"]:
                    del video[inst]
    zero = det["pred_masks"].new_zeros(det["pred_masks"].shape[-2:])
    cls = torch.stack([torch.stack([l for l in v["logits"] if l is not None]).mean(0) for v in video.values()])[None]
    dense = torch.stack([torch.stack([zero if m is None else m for m in v["masks"]]) for v in video.values()])[None]
    return cls, dense


def composed_postprocess(masks, s):
    """inference_video's loop over chunks of five instances x five frames: masks [K, F, h, w] -> bool [K, F, H, W], numerator, denominator."""
    outs, nums, dens = [], [], []
    for k in range(0, masks.shape[0], 5):
        part = masks[k:k + 5]
        num = torch.zeros(part.shape[0], device=masks.device)
        den = torch.zeros(part.shape[0], device=masks.device)
        chunks = []
        for i in range(0, part.shape[1], 5):
            t = F.interpolate(part[:, i:i + 5], size=s["padded"], mode="bilinear", align_corners=False)[:, :, :s["crop"][0], :s["crop"][1]]
            t = F.interpolate(t, size=s["out"], mode="bilinear", align_corners=False)
            m = (t > 0.0).float()
            num += (t.sigmoid() * m).flatten(1).sum(1)
            den += m.flatten(1).sum(1)
            chunks.append(m.bool())
        outs.append(torch.cat(chunks, dim=1))
        nums.append(num)
        dens.append(den)
    return torch.cat(outs), torch.cat(nums), torch.cat(dens)


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
    s = SMOKE if args.smoke else SHIPPED
    runs, warmup = (2, 1) if args.smoke else (10, 2)
    det = make_clip(s, dev)
    kw = dict(num_classes=s["C"])
    trk = sa.SimpleTracker(**kw)
    defaults = {k: getattr(trk, k) for k in ("inference_select_thr", "mask_nms_thr", "match_score_thr", "init_score_thr", "maximum_cache", "num_dead_frames",
                                               "noise_frame_num", "none_frame_num", "suppress_frame_num")}
    copies, real = [], vis._device_to_host
    vis._device_to_host = lambda t: (copies.append(1), real(t))[1]
    out = trk.inference(det, dense_masks=False)
    vis._device_to_host = real
    syncs = []
    cls, dense = composed_tracker(det, defaults, syncs)
    n_sync = len(syncs)
    K = out["mask_index"].shape[0]
    same = K == dense.shape[1] and bool((cls - out["pred_logits"]).abs().max() < 1e-4)
    lines = [f"shape: F {s['F']}, Q {s['Q']}, classes {s['C']}, E {s['E']}, masks {s['src']}, padded {s['padded']}, crop {s['crop']}, output {s['out']}, "
             f"top-k {s['topk']}; {K} instances tracked (composed path: {dense.shape[1]}; final logits agree: {same})"]
    nat_t = host_timed(lambda: trk.inference(det, dense_masks=False), warmup, runs)
    ref_t = host_timed(lambda: composed_tracker(det, defaults, []), warmup, runs)
    lines.append(f"(i) tracker, host clock, median (min, max) ms of {runs}: native {nat_t[0]:.2f} ({nat_t[1]:.2f}, {nat_t[2]:.2f}) with {len(copies)} "
                 f"host synchronisation; composed {ref_t[0]:.2f} ({ref_t[1]:.2f}, {ref_t[2]:.2f}) with {n_sync} host synchronisations; "
                 f"composed / native {ref_t[0] / nat_t[0]:.2f}")
    scores = vis.vis_scores(out["pred_logits"][0], full=True)[2]
    top = scores.flatten().topk(min(s["topk"], scores.numel()))[1] // s["C"]
    picked = out["mask_index"][top]
    gathered = vis.resample_masks(out["det_masks"], picked, s["src"], s["src"], s["src"], masks=False, logits=True, sums=False)["logits"]
    ws = torch.empty(sa._native.lib.sf_op_vis_postprocess_workspace_bytes(picked.shape[0], s["F"], *s["out"]), dtype=torch.uint8, device=dev)
    native_post = lambda: vis.resample_masks(out["det_masks"], picked, s["padded"], s["crop"], s["out"], workspace=ws)      # noqa: E731
    a, b = native_post(), composed_postprocess(gathered, s)
    differ = int((a["masks"] != b[0]).sum())
    nat_p = timed(native_post, warmup, runs)
    ref_p = timed(lambda: composed_postprocess(gathered, s), warmup, runs)
    out_bytes = picked.shape[0] * s["F"] * s["out"][0] * s["out"][1]
    lines.append(f"(ii) post-processing of {picked.shape[0]} instances, HIP events, median (min, max) ms of {runs}: native {nat_p[0]:.3f} ({nat_p[1]:.3f}, "
                 f"{nat_p[2]:.3f}), {out_bytes / nat_p[0] / 1e6:.1f} GB/s of bool output, no host synchronisation; composed {ref_p[0]:.3f} ({ref_p[1]:.3f}, "
                 f"{ref_p[2]:.3f}), no host synchronisation; composed / native {ref_p[0] / nat_p[0]:.2f}; bits differing {differ} of {out_bytes}, "
                 f"denominators {a['denominator'].tolist()} vs {b[2].long().tolist()}")
    print("\n".join(lines))
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "vis.txt")
        if not os.path.exists(path):                         # the first hardware run is the record; later runs print only
            with open(path, "w") as fh:
                fh.write("tools/vis_bench.py on an MI355X\n" + "\n".join(lines) + "\n")
            print("wrote", path)


if __name__ == "__main__":
    main()
