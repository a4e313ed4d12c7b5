"""Torch restatement, at a chosen dtype, of the reference's image inference after the mask decoder, in its order of operations: the
upsample to the padded size and ``sem_seg_postprocess`` of ``TimesformerMaskFormer.forward``'s eval branch, and its
``semantic_inference``, ``panoptic_inference`` and ``instance_inference`` (mask2former/timesformer_maskformer_model.py).  In fp64 it
reproduces fixture F26 (tests/golden/f26_seg.npz, written by tools/make_golden_seg.py from the reference's own functions); in fp32 it is
the precision floor of the tests.

The scenario (``make_scenario``, a pure function of the seed, every value exact in fp16): Q = 12 queries, C = 5 classes (things 0, 1, 2;
stuff 3, 4) + 1, masks 12 x 20, padded 48 x 80, the image 45 x 77, outputs 31 x 50 ("down") and 75 x 130 ("up").  Planted: queries 0 and
1 are two stuff regions of class 3 that merge into one segment; query 2 scores 0.47, under ``object_mask_threshold`` = 0.5; query 3 (and 9,
10, 11) is a no-object query; query 4 is a large thing; query 5 is a kept thing mostly occluded by 4 (it wins a twelfth of its own area,
under ``overlap_threshold`` = 0.5, and is dropped); query 6 is a kept thing that lies inside 4, has a lower score and a background of -20,
and wins no pixel; queries 7 and 8 are two things that overlap in one column and both survive.  The second case, ``nothing``, raises
``object_mask_threshold`` to 0.99, above every score.

Every decision that a rounding could flip is recorded as a margin relative to the larger operand (score against the threshold, the
area ratio against ``overlap_threshold``, the gaps of the top-k); F26's smallest is at least MIN_MARGIN = 1e-3.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import vis_oracle as VO
from tests.helpers import EPS32, MARGIN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f26_seg.npz")
MIN_MARGIN = 1e-3
SEED = 26
QUERIES, CLASSES, MASK_H, MASK_W = 12, 5, 12, 20
THINGS = (0, 1, 2)
TOPK = 6
GEOMETRIES = {"down": dict(padded=(48, 80), crop=(45, 77), out=(31, 50)), "up": dict(padded=(48, 80), crop=(45, 77), out=(75, 130))}
CASES = {"planted": dict(num_classes=CLASSES, object_mask_threshold=0.5, overlap_threshold=0.5, thing_classes=THINGS),
         "nothing": dict(num_classes=CLASSES, object_mask_threshold=0.99, overlap_threshold=0.5, thing_classes=THINGS)}


def make_scenario(seed=SEED):
    """(mask_cls [Q, C + 1], mask_pred [Q, 12, 20]) fp32 holding fp16-exact values."""
    rs = np.random.RandomState(seed)
    Q, C = QUERIES, CLASSES
    logits = np.zeros((Q, C + 1), np.float32)
    logits[:, :C] = -3.0 - 0.25 * np.arange(C)
    logits[:, C] = 3.0
    masks = -10.0 + 0.25 * rs.randint(-8, 9, size=(Q, MASK_H, MASK_W)).astype(np.float32)
    # (query, class, logit, rows, columns)
    objects = [(0, 3, 4.0, (0, 6), (0, 10)), (1, 3, 3.5, (0, 6), (10, 20)), (2, 0, 0.25, (2, 5), (4, 9)), (4, 0, 4.25, (6, 12), (0, 12)),
               (5, 1, 2.0, (6, 12), (2, 13)), (6, 2, 1.5, (7, 10), (3, 7)), (7, 1, 3.75, (6, 12), (13, 17)), (8, 2, 3.0, (6, 12), (16, 20))]
    for q, cls, level, (r0, r1), (c0, c1) in objects:
        logits[q, :C] = -2.0 - 0.25 * ((np.arange(C) - cls) % C)
        logits[q, cls] = level
        logits[q, C] = 0.0
        if q == 6:
            masks[q] -= 10.0                                 # a background of -20: it wins nothing outside query 4's region either
        masks[q, r0:r1, c0:c1] += 20.0
    for v in (logits, masks):
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
    return torch.from_numpy(logits), torch.from_numpy(masks)


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def to_padded(mask_pred, geometry):
    """forward's upsample of the decoder's masks to the padded batch size."""
    return F.interpolate(mask_pred[None], size=tuple(geometry["padded"]), mode="bilinear", align_corners=False)[0]


def sem_seg_postprocess(result, img_size, output_height, output_width):
    """detectron2's function: crop to the image, resize to the output."""
    result = result[:, :img_size[0], :img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


def resample(mask_pred, geometry):
    """The masks as the three functions see them with sem_seg_postprocess before inference: [Q, H, W]."""
    return sem_seg_postprocess(to_padded(mask_pred, geometry), geometry["crop"], *geometry["out"])


def semantic(mask_cls, mask_pred, geometry, before=True, dtype=torch.float64):
    """semantic_inference in either order of forward's eval branch -> [C, H, W]."""
    cls, m = mask_cls.to(dtype), to_padded(mask_pred.to(dtype), geometry)
    if before:
        m = sem_seg_postprocess(m, geometry["crop"], *geometry["out"])
    sem = torch.einsum("qc,qhw->chw", F.softmax(cls, dim=-1)[..., :-1], m.sigmoid())
    return sem if before else sem_seg_postprocess(sem, geometry["crop"], *geometry["out"])


def panoptic(mask_cls, mask_pred, geometry, kw, dtype=torch.float64, given=None):
    """panoptic_inference over the resampled masks.  Returns the map, segments_info, per query its segment id and its three counts
    (mask_area, original_area, both; zeros for a query that is not kept), the per-pixel winner (-1: nothing kept) and what the tests
    need to tell decided pixels: ``prob`` [Q, H, W] (score x sigmoid, -inf for a query that is not kept) and ``r`` [Q, H, W]."""
    cls, r = mask_cls.to(dtype), resample(mask_pred.to(dtype), geometry)
    Q = cls.shape[0]
    scores, labels = F.softmax(cls, dim=-1).max(-1) if given is None else (given[0].to(dtype), given[1].long())      # given: (scores, labels) [Q]
    sig = r.sigmoid()
    keep = labels.ne(kw["num_classes"]) & (scores > kw["object_mask_threshold"])
    margins = [("score", _rel(s, kw["object_mask_threshold"])) for s, l in zip(scores, labels) if int(l) != kw["num_classes"]]
    kept = torch.nonzero(keep).flatten().tolist()
    H, W = r.shape[-2:]
    pan = torch.zeros((H, W), dtype=torch.int32)
    winner = torch.full((H, W), -1, dtype=torch.long)
    prob = torch.full((Q, H, W), float("-inf"), dtype=dtype)
    counts = np.zeros((Q, 3), np.int64)
    info, seg_of = [], [0] * Q
    if kept:
        prob[keep] = scores[keep].view(-1, 1, 1) * sig[keep]
        ids = prob[keep].argmax(0)
        winner = torch.tensor(kept)[ids]
        stuff, current = {}, 0
        for k, q in enumerate(kept):
            pred_class = int(labels[q])
            isthing = pred_class in kw["thing_classes"]
            mask_area = int((ids == k).sum())
            original_area = int((sig[q] >= 0.5).sum())
            mask = (ids == k) & (sig[q] >= 0.5)
            counts[q] = (mask_area, original_area, int(mask.sum()))
            if mask_area > 0 and original_area > 0 and int(mask.sum()) > 0:
                margins.append(("overlap", _rel(mask_area / original_area, kw["overlap_threshold"])))
                if mask_area / original_area < kw["overlap_threshold"]:
                    continue
                if not isthing:
                    if pred_class in stuff:
                        pan[mask] = stuff[pred_class]
                        seg_of[q] = stuff[pred_class]
                        continue
                    stuff[pred_class] = current + 1
                current += 1
                pan[mask] = current
                seg_of[q] = current
                info.append({"id": current, "isthing": bool(isthing), "category_id": pred_class})
    return {"map": pan, "segments_info": info, "segment_of_query": seg_of, "counts": counts, "winner": winner, "scores": scores, "labels": labels,
            "prob": prob, "r": r, "margins": margins}


def bands(p64, p32):
    """The bands of a panoptic case from its fp64 and fp32 runs: MARGIN x max(measured fp32 floor, eps32 x max |value|), for
    score x sigmoid and for r."""
    kept = torch.isfinite(p64["prob"])
    fp = float((p32["prob"][kept].double() - p64["prob"][kept]).abs().max()) if kept.any() else 0.0
    band_prob = MARGIN * max(fp, EPS32 * (float(p64["prob"][kept].abs().max()) if kept.any() else 0.0))
    band_r = MARGIN * max(float((p32["r"].double() - p64["r"]).abs().max()), EPS32 * float(p64["r"].abs().max()))
    return band_prob, band_r


def undecided(pan64, band_prob, band_r):
    """Pixels of a panoptic result (fp64) that a rounding may decide otherwise: the gap between the best and the second-best
    score x sigmoid, or |r| of the winner, is inside its band.  All False when nothing is kept."""
    prob, r, winner = pan64["prob"], pan64["r"], pan64["winner"]
    if int(winner.max()) < 0:
        return torch.zeros(winner.shape, dtype=torch.bool)
    top = torch.sort(prob, 0, descending=True)[0]
    gap = top[0] - top[1] if prob.shape[0] > 1 else torch.full(winner.shape, float("inf"), dtype=prob.dtype)
    gap = torch.where(torch.isfinite(gap), gap, torch.full_like(gap, float("inf")))      # one kept query: nothing to confuse it with
    rw = r.gather(0, winner.clamp(min=0)[None])[0]
    return ~((gap > band_prob) & (rw.abs() > band_r))


def overlap_decisions_hold(pan64, kw, slack):
    """Every overlap decision keeps its side when each area moves by ``slack`` pixels against it."""
    for mask_area, original_area, both in pan64["counts"].tolist():
        if mask_area > 0 and original_area > 0 and both > 0:
            below = mask_area / original_area < kw["overlap_threshold"]
            worst = (mask_area + slack) / max(original_area - slack, 1) if below else max(mask_area - slack, 0) / (original_area + slack)
            if (worst < kw["overlap_threshold"]) != below:
                return False
    return True


def instance(mask_cls, mask_pred, geometry, num_classes=CLASSES, topk=TOPK, things=None, dtype=torch.float64):
    """instance_inference over the resampled masks, sorted by class score (the reference's topk is unsorted: compare as sets of rows)."""
    cls, r = mask_cls.to(dtype), resample(mask_pred.to(dtype), geometry)
    scores = F.softmax(cls, dim=-1)[:, :-1]
    flat = scores.flatten(0, 1)
    top_scores, top = flat.topk(topk, sorted=True)
    margins = [("topk", _rel(top_scores[i], top_scores[i + 1])) for i in range(topk - 1)]
    rest = flat.clone()
    rest[top] = -1
    margins.append(("topk", _rel(top_scores[-1], rest.max())))
    labels, rows = top % num_classes, top // num_classes
    if things is not None:
        keep = torch.tensor([int(l) in things for l in labels])
        top_scores, labels, rows = top_scores[keep], labels[keep], rows[keep]
    m = r[rows]
    on = (m > 0).float()                                     # the reference's .float(): the denominator and its + 1e-6 are fp32 at any dtype
    mask_scores = (m.sigmoid().flatten(1) * on.flatten(1)).sum(1) / (on.flatten(1).sum(1) + 1e-6)
    return {"scores": top_scores * mask_scores, "labels": labels, "rows": rows, "masks": m > 0, "logits": m, "margins": margins}


# the kernels alone: source 23 x 37 on the two geometries of the video fixture
KERNEL_Q, KERNEL_C = (1, 5, 100), (1, 17, 133)
PAN_Q = (1, 7, 100)
PAN_THRESHOLD = 0.35


def make_kernel_masks(Q, seed):
    """[Q, 23, 37] fp32: a background of -10 with noise of up to 2 (multiples of 1/4) and a blob of +10 per query, the magnitude of real
    mask logits.  Query 0 is +6 with the same noise everywhere: every pixel has a query with a clearly positive logit, so that the
    panoptic winner is decided by scores that differ in the third digit and not by the noise of a background that nobody claims."""
    rs = np.random.RandomState(seed)
    h, w = VO.MASK_H, VO.MASK_W
    m = -10.0 + 0.25 * rs.randint(-8, 9, size=(Q, h, w)).astype(np.float32)
    for q in range(Q):
        y, x = rs.randint(0, h - 4), rs.randint(0, w - 6)
        m[q, y:y + rs.randint(3, h - y + 1), x:x + rs.randint(4, w - x + 1)] += 20.0
    m[0] = 6.0 + 0.25 * rs.randint(-8, 9, size=(h, w)).astype(np.float32)
    return torch.from_numpy(m)


def make_kernel_logits(Q, C, seed):
    return torch.from_numpy((3 * np.random.RandomState(seed).standard_normal((Q, C + 1))).astype(np.float32))


def make_panoptic_inputs(Q, num_classes=CLASSES):
    """(masks, scores fp32 [Q], labels int32 [Q]) for the argmax kernel alone: distinct scores 0.36 .. 0.98 in a seeded order with
    query 0, the full cover, the lowest; every fifth query (from 3) is a no-object query and every seventh (from 5) scores 0.2, under
    PAN_THRESHOLD."""
    rs = np.random.RandomState(2600 + Q)
    scores = np.linspace(0.36, 0.98, Q).astype(np.float32)
    scores[1:] = rs.permutation(scores[1:])
    labels = rs.randint(0, num_classes, size=Q).astype(np.int32)
    for q in range(1, Q):
        if q % 5 == 3:
            labels[q] = num_classes
        if q % 7 == 5:
            scores[q] = 0.2
    return make_kernel_masks(Q, 2600 + Q), torch.from_numpy(scores), torch.from_numpy(labels)


def panoptic_alone(Q, geometry, dtype=torch.float64, threshold=PAN_THRESHOLD):
    masks, scores, labels = make_panoptic_inputs(Q)
    kw = dict(num_classes=CLASSES, object_mask_threshold=threshold, overlap_threshold=0.5, thing_classes=THINGS)
    return panoptic(torch.zeros(Q, CLASSES + 1), masks, geometry, kw, dtype=dtype, given=(scores, labels))


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def info_array(segments_info):
    """segments_info as int32 [n, 3]: id, isthing, category_id."""
    return np.array([[s["id"], int(s["isthing"]), s["category_id"]] for s in segments_info], np.int32).reshape(-1, 3)


pack_bits = VO.pack_bits
