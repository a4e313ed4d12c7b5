"""fp64 restatement of the reference's video-instance-segmentation inference after the mask decoder, in its order of operations: the
per-frame selection and ``mask_nms`` (ctvis/utils/utils.py), ``SimpleTracker`` with its ``MemoryBank`` and ``Tracklet``
(ctvis/modeling/tracker/) and ``CTVISModel.inference_video`` (ctvis/ctvis_model.py).  It reproduces fixture F25
(tests/golden/f25_vis.npz, written by tools/make_golden_vis.py from the reference itself) and records the MARGIN of every comparison that
decides something, relative to the larger operand: score - thr for ``inference_select_thr`` and ``init_score_thr``, the gaps of the
score sort among the selected detections, IoU - ``mask_nms_thr``, match_score - ``match_score_thr``, and best minus runner-up of every
``max`` / ``topk`` that picks an index.  F25's smallest margin is at least MIN_MARGIN = 1e-3: thousands of fp32 roundings, so an fp32
implementation must take every decision the same way.

The scenario (``make_scenario``, seeded, every value exact in fp16): F = 12 frames, Q = 12 queries, 5 classes + 1, E = 32, masks
23 x 37 (851 pixels: a ragged last word).  Planted: A (query 0) crosses the frame, its duplicate (query 6) is removed by NMS; B (query 1)
vanishes in frames 4-5 and returns inside ``num_dead_frames``, with a duplicate (query 7) in its first frames; C (query 2) stops after
frame 2 and its tracklet dies; D (query 3) lives for frames 5-6 only and is deleted by the noise rule; E (query 4) has an embedding
correlated with A's (cosine 0.6: under the cosine metric two tracklets pass the threshold and the ``frame_weight`` rule fires); a faint
detection (query 5) is selected but neither matched nor started.  In frame 5, while B is away and C's tracklet still lives, two
one-frame detections set greedy and Hungarian matching apart: X (query 9, embedding 0.625 B + 0.5 C, the higher score) and Y (query 10,
0.5 B).  Greedy gives B's tracklet to X, which comes first, and Y starts a track that the noise rule deletes; the assignment gives B's
tracklet to Y and C's to X, which keeps C alive for three more frames.  The other queries are background.

The alternatives must not pass by accident: tools/make_golden_vis.py asserts that every case differs from the default in something the
tests compare (ids and index table for hungarian, the memory bank's embeddings for the three other embed types, the match-score
matrices for cosine, the final logits for max), and the per-frame memory-bank embeddings (the reference's own, recorded from
``MemoryBank.exist_reid_embeds``) and match-score matrices are part of what ``track`` returns.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f25_vis.npz")
MIN_MARGIN = 1e-3
FRAMES, QUERIES, CLASSES, EMBED, MASK_H, MASK_W = 12, 12, 5, 32, 23, 37
SEED = 25
NUM_TOPK = 4

BASE = dict(num_classes=CLASSES, match_metric="bisoftmax", frame_weight=True, match_score_thr=0.45, temporal_score_type="mean", match_type="greedy",
            inference_select_thr=0.1, init_score_thr=0.3, mask_nms_thr=0.6, num_dead_frames=3, embed_type="similarity_guided", maximum_cache=3,
            noise_frame_num=4, noise_frame_ratio=0.4, suppress_frame_num=3, none_frame_num=2)
CASES = {"default": {}, "cosine": {"match_metric": "cosine"}, "hungarian": {"match_type": "hungarian"}, "last": {"embed_type": "last"},
         "weighted": {"embed_type": "temporally_weighted_softmax"}, "momentum": {"embed_type": "momentum"}, "max": {"temporal_score_type": "max"}}
# source 23 x 37 -> padded -> crop -> output
GEOMETRIES = {"down": dict(padded=(92, 148), crop=(90, 145), out=(67, 111)), "up": dict(padded=(92, 148), crop=(90, 145), out=(180, 290))}


def tracker_kwargs(case):
    return dict(BASE, **CASES[case])


def make_scenario():
    """pred_logits [F, Q, C + 1], pred_masks [F, Q, 23, 37], pred_embeds and pred_queries [F, Q, E], fp32 holding fp16-exact values."""
    rs = np.random.RandomState(SEED)
    Fr, Q, C1, E = FRAMES, QUERIES, CLASSES + 1, EMBED
    logits = np.zeros((Fr, Q, C1), np.float32)
    logits[..., :CLASSES] = -3.0 - 0.25 * np.arange(CLASSES)
    logits[..., CLASSES] = 3.0
    masks = -10.0 + 0.25 * rs.randint(-8, 9, size=(Fr, Q, MASK_H, MASK_W)).astype(np.float32)
    embeds = rs.randint(-4, 5, size=(Fr, Q, E)).astype(np.float32) / 16
    queries = rs.randint(-16, 17, size=(Fr, Q, E)).astype(np.float32) / 8
    bases = np.zeros((6, E), np.float32)
    for k in range(6):
        bases[k, 5 * k:5 * k + 5] = 2.0 * rs.choice([-1.0, 1.0], size=5)
    bases[4] += 0.75 * bases[0]
    # object: (query, class, logit, frames, rows, first column as a function of the frame, width, base embedding)
    objects = [(0, 0, 4.0, range(12), (2, 11), lambda f: 2 + f, 11, 0), (6, 0, 3.0625, range(12), (2, 11), lambda f: 3 + f, 11, 0),
               (1, 1, 3.5, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11], (12, 21), lambda f: 20 - f, 11, 1), (7, 1, 1.3125, range(4), (12, 21), lambda f: 21 - f, 11, 1),
               (2, 2, 2.75, range(3), (1, 7), lambda f: 25, 9, 2), (3, 3, 2.25, [5, 6], (14, 21), lambda f: 2, 7, 3),
               (4, 4, 1.75, range(12), (8, 15), lambda f: 14, 7, 4), (5, 2, -1.0, range(12), (0, 4), lambda f: 0, 4, 5),
               (9, 4, 3.75, [5], (0, 5), lambda f: 10, 7, 0.625 * bases[1] + 0.5 * bases[2]), (10, 0, 2.5, [5], (17, 22), lambda f: 29, 7, 0.5 * bases[1])]
    for n, (q, cls, level, frames, (r0, r1), col, width, base) in enumerate(objects):
        for f in frames:
            logits[f, q, :CLASSES] = -2.0 - 0.25 * ((np.arange(CLASSES) - cls) % CLASSES)
            logits[f, q, cls] = level + 0.125 * ((f * (n + 1)) % 3) * (level > 0)
            logits[f, q, CLASSES] = 0.0
            masks[f, q, r0:r1, col(f):col(f) + width] += 20.0
            if isinstance(base, int):
                embeds[f, q] += bases[base]
            else:
                embeds[f, q] = base                          # exact, without the per-frame perturbation
    out = {"pred_logits": logits, "pred_masks": masks, "pred_embeds": embeds, "pred_queries": queries}
    for k, v in out.items():
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v), k
    return {k: torch.from_numpy(v) for k, v in out.items()}


def pack_bits(m):
    """bool [..., P] -> uint32 words [..., ceil(P / 32)], bit p & 31 of word p / 32."""
    m = np.asarray(m, bool)
    P = m.shape[-1]
    pad = np.zeros(m.shape[:-1] + ((-P) % 32,), bool)
    b = np.concatenate([m, pad], -1).reshape(m.shape[:-1] + (-1, 32))
    return (b.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words, P):
    w = np.asarray(words).astype(np.uint32)
    b = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(w.shape[:-1] + (-1,))[..., :P].astype(bool)


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def front(det, dtype=torch.float64):
    """What the kernels compute per frame: max scores, labels, ``x > 0`` bits, areas and intersections (integers)."""
    logits = det["pred_logits"].to(dtype)
    scores = F.softmax(logits, dim=-1)[..., :-1]
    mx, lab = scores.max(-1)
    bits = (det["pred_masks"] > 0).flatten(2)
    b = bits.to(torch.int64)
    return {"scores": scores, "max_scores": mx, "labels": lab, "bits": bits, "area": b.sum(-1), "inter": b @ b.transpose(1, 2)}


class _Tracklet:
    def __init__(self):
        self.scores, self.embeds, self.frame_ids, self.exist_frames = [], [], [], 0
        self.last = self.guided = None


def track(det, kw, dtype=torch.float64):
    """The reference's SimpleTracker.inference.  Returns the per-frame selections, the instances and the recorded margins."""
    fr = front(det, dtype)
    logits_all, embeds_all = det["pred_logits"].to(dtype), det["pred_embeds"].to(dtype)
    Fr, Q = logits_all.shape[:2]
    margins = []
    note = lambda what, a, b: margins.append((what, _rel(a, b)))      # noqa: E731
    bank, num_tracklets, video = {}, 0, {}
    selected_f, kept_f, ids_f, tracked_f, bank_ids_f, bank_embeds_f, match_f = [], [], [], [], [], [], []
    for f in range(Fr):
        mx = fr["max_scores"][f]
        order = torch.sort(mx, dim=0, descending=True)[1]
        sc = mx[order]
        valid = sc > kw["inference_select_thr"]
        if valid.sum() == 0:
            valid[0] = True
        for s in sc:
            note("select", s, kw["inference_select_thr"])
        n_valid = int(valid.sum())
        for i in range(n_valid):                              # the sort's order among the selected, and against the first one left out
            if i + 1 < len(sc):
                note("sort", sc[i], sc[i + 1])
        srt = torch.sort(fr["scores"][f], dim=-1, descending=True)[0]
        for q in order[:n_valid].tolist():
            if srt.shape[-1] > 1:
                note("label", srt[q, 0], srt[q, 1])
        order, sc = order[valid], sc[valid]
        selected_f.append(order.tolist())
        keep = [True] * len(order)
        for i in range(len(order) - 1):
            if not keep[i]:
                continue
            for j in range(i + 1, len(order)):
                if not keep[j]:
                    continue
                qi, qj = int(order[i]), int(order[j])
                inter = int(fr["inter"][f, qi, qj])
                union = int(fr["area"][f, qi]) + int(fr["area"][f, qj]) - inter
                iou = (inter + 1e-6) / (union + 1e-6)
                note("nms", iou, kw["mask_nms_thr"])
                if iou > kw["mask_nms_thr"]:
                    keep[j] = False
        keep = torch.tensor(keep)
        order, sc = order[keep], sc[keep]
        kept_f.append(order.tolist())
        emb, lg = embeds_all[f][order], logits_all[f][order]
        ids = torch.full((len(order),), -1, dtype=torch.long)
        bank_ids_f.append(list(bank) if num_tracklets > 0 else [])
        bank_embeds_f.append(None)
        match_f.append(None)
        if num_tracklets > 0 and bank:
            exist_ids = list(bank)
            exist_emb = []
            for t in bank.values():
                if kw["embed_type"] == "temporally_weighted_softmax":
                    w = torch.stack(t.scores)
                    n = w.shape[0]
                    count = int(np.floor(1.0 / (1 / n) + 1)) - 1
                    temporal = torch.tensor([(i + 1) * (1 / n) for i in range(count)], dtype=torch.float64).to(torch.float32).to(w)
                    w = w + temporal
                    exist_emb.append((torch.stack(t.embeds) * w.unsqueeze(1)).sum(0) / w.sum())
                else:
                    exist_emb.append({"last": t.embeds[-1], "momentum": t.last, "similarity_guided": t.guided}[kw["embed_type"]])
            exist_emb = torch.stack(exist_emb, dim=0)
            exist_frames = torch.tensor([t.exist_frames for t in bank.values()], dtype=torch.long)
            if kw["match_metric"] == "bisoftmax":
                sim = torch.mm(emb, exist_emb.t())
                match = (sim.softmax(dim=1) + sim.softmax(dim=0)) / 2
            else:
                match = torch.mm(F.normalize(emb, p=2, dim=1), F.normalize(exist_emb, p=2, dim=1).t())
            thr = kw["match_score_thr"]
            bank_embeds_f[-1], match_f[-1] = exist_emb, match.clone()
            if kw["match_type"] == "greedy":
                for i in range(len(order)):
                    row = match[i].clone()
                    above = row > thr
                    for v in row:
                        note("match>thr", v, thr)
                    if kw["frame_weight"] and int(above.sum()) > 1:
                        w = exist_frames[above].to(row)
                        row[above] = row[above] * w
                        row[~above] = row[~above] * w.mean()
                    best, col = torch.max(row, dim=0)
                    if len(row) > 1:
                        top2 = torch.topk(row, 2)[0]
                        if float(top2[0]) > thr:              # the argmax decides something only where the best passes
                            note("argmax", top2[0], top2[1])
                    note("match", best, thr)
                    if best > thr:
                        ids[i] = exist_ids[int(col)]
                        match[:i, col] = 0
                        match[i + 1:, col] = 0
            else:
                from scipy.optimize import linear_sum_assignment
                rows, cols = linear_sum_assignment(-match.numpy())
                for r, c in zip(rows, cols):
                    note("match", match[r, c], thr)
                    if not match[r, c] < thr:
                        ids[r] = exist_ids[c]
        for s in sc[ids == -1]:
            note("init", s, kw["init_score_thr"])
        new = (ids == -1) & (sc > kw["init_score_thr"])
        ids[new] = torch.arange(num_tracklets, num_tracklets + int(new.sum()), dtype=torch.long)
        num_tracklets += int(new.sum())
        ok = ids > -1
        ids_f.append(ids[ok].tolist())
        tracked_f.append(order[ok].tolist())
        for k in torch.nonzero(ok).flatten().tolist():
            inst = int(ids[k])
            t = bank.setdefault(inst, _Tracklet())
            t.scores.append(sc[k])
            t.embeds.append(emb[k])
            t.frame_ids.append(f)
            if t.exist_frames == 0:
                t.last = t.guided = emb[k]
            else:
                t.last = (1 - 0.75) * t.last + 0.75 * emb[k]
                earlier = torch.stack(t.embeds[:-1], dim=0)
                sim = torch.sum(torch.einsum("bc,c->b", F.normalize(earlier, dim=-1), F.normalize(emb[k], dim=-1))) / (len(t.embeds) - 1)
                beta = max(0, sim)
                t.guided = (1 - beta) * t.guided + beta * emb[k]
            t.exist_frames += 1
            if len(t.scores) > kw["maximum_cache"]:
                t.scores.pop(0)
                t.embeds.pop(0)
            entry = video.setdefault(inst, {"rows": [None] * f, "logits": [None] * f})
            entry["rows"].append(f * Q + int(order[k]))
            entry["logits"].append(lg[k])
        for dead in [i for i, t in bank.items() if f - t.frame_ids[-1] > kw["num_dead_frames"]]:
            del bank[dead]
        for v in video.values():
            if len(v["rows"]) < f + 1:
                v["rows"].append(None)
                v["logits"].append(None)
        if f > kw["noise_frame_num"]:
            for inst in list(video):
                rows = video[inst]["rows"]
                present = sum(r is not None for r in rows)
                trailing = 0
                for r in rows[::-1]:
                    if r is not None:
                        break
                    trailing += 1
                if trailing >= kw["none_frame_num"] and present < kw["suppress_frame_num"]:
                    del video[inst]
    final, index = [], []
    for v in video.values():
        seen = torch.stack([l for l in v["logits"] if l is not None])
        final.append(seen.mean(0) if kw["temporal_score_type"] == "mean" else seen.max(0)[0])
        index.append([-1 if r is None else r for r in v["rows"]])
    return {"selected": selected_f, "kept": kept_f, "ids": ids_f, "tracked": tracked_f, "instances": list(video),
            "bank_ids": bank_ids_f, "bank_embeds": bank_embeds_f, "match": match_f,
            "index": np.array(index, np.int32).reshape(len(index), Fr), "logits": torch.stack(final) if final else torch.zeros(0, logits_all.shape[-1], dtype=dtype),
            "margins": margins}


def dense_masks(det, index, dtype=torch.float64):
    """[K, F, h, w]: the rows the index table names, zeros where it holds -1 (the reference's zero mask)."""
    flat = det["pred_masks"].to(dtype).flatten(0, 1)
    idx = torch.from_numpy(np.asarray(index)).long()
    out = flat[idx.clamp(min=0)]
    out[idx < 0] = 0
    return out


def resample(masks, padded, crop, out):
    """inference_video's two F.interpolate calls with the crop between them, in ``masks``' dtype."""
    x = F.interpolate(masks, size=tuple(padded), mode="bilinear", align_corners=False)
    x = x[:, :, :crop[0], :crop[1]]
    return F.interpolate(x, size=tuple(out), mode="bilinear", align_corners=False)


def inference_video(logits, masks, geometry, num_classes=CLASSES, num_topk=NUM_TOPK):
    """``logits`` [K, C + 1], ``masks`` [K, F, h, w] -> top-k scores, labels, instance rows, the resampled logits, bool masks, sums; and
    the top-k's margins."""
    scores = F.softmax(logits, dim=-1)[:, :-1]
    flat = scores.flatten(0, 1)
    top_scores, top = flat.topk(num_topk, sorted=True)
    margins = [("topk", _rel(top_scores[i], top_scores[i + 1])) for i in range(num_topk - 1)]
    rest = flat.clone()
    rest[top] = -1
    if num_topk < flat.numel():
        margins.append(("topk", _rel(top_scores[-1], rest.max())))
    labels = top % num_classes
    rows = top // num_classes
    res = resample(masks[rows], geometry["padded"], geometry["crop"], geometry["out"])
    m = (res > 0).to(res.dtype)
    numerator = (res.sigmoid() * m).flatten(1).sum(1)
    denominator = m.flatten(1).sum(1)
    # the reference's accumulators are fp32 whatever the masks' dtype, filled per chunk of five frames: its scores carry those roundings
    num32, den32 = torch.zeros(len(rows), dtype=torch.float32), torch.zeros(len(rows), dtype=torch.float32)
    for i in range(0, res.shape[1], 5):
        num32 += (res[:, i:i + 5].sigmoid() * m[:, i:i + 5]).flatten(1).sum(1)
        den32 += m[:, i:i + 5].flatten(1).sum(1)
    return {"scores": top_scores * (num32 / (den32 + 1e-6)), "topk_scores": top_scores, "labels": labels, "rows": rows, "logits": res,
            "masks": res > 0, "numerator": numerator, "denominator": denominator, "margins": margins}


# the post-processing kernel's cases: F25's two geometries, a downscale whose source box nearly fills the LDS a tile may take, an exact 2x with crop == padded (16-byte bool stores), a crop == padded case
# whose width is a multiple of 4 only (float4 logits, byte masks); K in {1, 3}, F in {1, 5}, absent entries in every one with K F > 1
POST_CASES = {"down": dict(GEOMETRIES["down"], src=(MASK_H, MASK_W), K=3, F=5), "up": dict(GEOMETRIES["up"], src=(MASK_H, MASK_W), K=1, F=5),
              "x2": dict(src=(12, 20), padded=(24, 40), crop=(24, 40), out=(48, 80), K=3, F=1),
              "nocrop": dict(src=(MASK_H, MASK_W), padded=(92, 148), crop=(92, 148), out=(70, 120), K=1, F=1),
              # one 16 x 256 output tile reaches the whole 48 x 300 source: 58 KB of LDS, close to the 63 KB a tile's box may take
              "shrink": dict(src=(48, 300), padded=(48, 300), crop=(48, 300), out=(16, 256), K=1, F=2)}


def make_post_inputs(name):
    """(det_masks [R, h, w] fp32, index [K, F] int32) of a post-processing case: blobs of +-10 with noise of up to 2 (the magnitude of real
    mask logits; multiples of 1/4), R = K F + 2 rows, and absent entries."""
    c = POST_CASES[name]
    rs = np.random.RandomState(2500 + sorted(POST_CASES).index(name))
    (h, w), K, Fr = c["src"], c["K"], c["F"]
    R = K * Fr + 2
    m = -10.0 + 0.25 * rs.randint(-8, 9, size=(R, h, w)).astype(np.float32)
    for r in range(R):
        y, x = rs.randint(0, h - 4), rs.randint(0, w - 6)
        m[r, y:y + rs.randint(3, h - y + 1), x:x + rs.randint(4, w - x + 1)] += 20.0
    index = rs.permutation(R)[:K * Fr].reshape(K, Fr).astype(np.int32)
    if K * Fr > 1:
        index[-1, -1] = -1
        index[0, Fr // 2] = -1
    return torch.from_numpy(m), torch.from_numpy(index)


def post_reference(det_masks, index, c, dtype=torch.float64):
    """The two-step composition on the gathered planes -> (logits [K, F, H, W], numerator [K], denominator [K])."""
    idx = index.long()
    planes = det_masks.to(dtype)[idx.clamp(min=0)]
    planes[idx < 0] = 0
    res = resample(planes, c["padded"], c["crop"], c["out"])
    on = (res > 0).to(dtype)
    return res, (res.sigmoid() * on).flatten(1).sum(1), on.flatten(1).sum(1)


def check_trace(trace, case, golden, det, check):
    """A tracker's per-frame ``trace`` against F25 and the oracle: selections, kept sets, ids and the memory bank's ids exactly; the
    memory bank's embeddings (F25 holds the reference's own) and the match-score matrices (the oracle's, which F25's embeddings pin)
    through ``check`` = helpers.check_against_floor, with the oracle in fp32 as the floor.  This is what tells the alternatives of
    ``match_metric`` and ``embed_type`` apart where they lead to the same ids."""
    kw = tracker_kwargs(case)
    for k in ("selected", "kept", "ids", "bank_ids"):
        assert [t[k] for t in trace] == unragged(golden[f"{case}.{k}"]), (case, k)
    want = track({k: v.double() for k, v in det.items()}, kw)
    floor = track(det, kw, dtype=torch.float32)
    frames = [f for f, t in enumerate(trace) if t["match"] is not None]
    assert frames == [f for f, m in enumerate(want["match"]) if m is not None] and len(frames) >= len(trace) - 1
    cat = lambda xs: torch.cat([x.flatten() for x in xs])      # noqa: E731
    stored = golden[f"{case}.bank_embeds"]
    ref_embeds = cat([torch.from_numpy(stored[f, :len(trace[f]["bank_ids"])]) for f in frames])
    assert all(trace[f]["bank_embeds"].shape == want["bank_embeds"][f].shape and trace[f]["match"].shape == want["match"][f].shape for f in frames)
    check(f"{case} memory-bank embeddings", cat([trace[f]["bank_embeds"] for f in frames]), cat([floor["bank_embeds"][f] for f in frames]), ref_embeds)
    check(f"{case} match scores", cat([trace[f]["match"] for f in frames]), cat([floor["match"][f] for f in frames]), cat([want["match"][f] for f in frames]))


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def ragged(lists):
    """A list of int lists as one array, rows padded with -2 (ids and query indices are >= -1)."""
    n = max([len(l) for l in lists] + [1])
    return np.array([list(l) + [-2] * (n - len(l)) for l in lists], np.int32)


def unragged(a):
    return [[int(v) for v in row if v != -2] for row in a]
