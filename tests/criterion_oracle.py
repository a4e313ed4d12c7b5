"""Oracle of the Mask2Former criterion (streamformer_amd/criterion.py): HungarianMatcher and SetCriterion restated in torch, in the
reference's operator order and in any dtype (``point_sample`` as ``F.grid_sample``, the rule of ``get_uncertain_point_coords_with_randomness``,
the batch and pair losses, the matcher with scipy), plus the planted scenario of fixture F27 (tools/make_golden_criterion.py pins this file
to the reference) and the three conditions on it: agreement, assignment margin, undecided points.

Every input is a pure function of a seed, made with numpy's PCG64 and arithmetic only, and is exactly representable in fp32, so that the
fp64 oracle, the fp32 oracle and the kernels start from the same numbers.  The ``torch.rand`` draws are planted: ``draws(case)`` lists
them in the reference's order (per layer: one [1, K, 2] per image for the matcher, then [N, int(K * oversample), 2] and, when
K - int(importance * K) > 0, [N, that, 2] for the losses) and ``Queue`` hands them out.

F27 (tests/golden/f27_criterion.npz), measured when it was written: smallest assignment margin 6.8e-3 of the largest |cost|; largest share of
undecided points of a pair 6.7e-3 (1 of 150: the threshold point itself).  ``EXTRA`` holds the cases whose draws are too large to store:
the generator compares them with the reference all the same, and they meet the same conditions (margins 1.5e-3 to 2.6e-1, shares up to
6.7e-3).
"""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

EPS32 = 2.0 ** -24
CAP = 1e-2              # share of undecided points a pair may have (CAP of tests/test_seg.py)
MARGIN_REL = 1e-3       # assignment margin relative to the largest |cost| (the F25 / F26 convention)

BASE = dict(L=3, B=3, G=(3, 0, 5), Q=20, C=7, pred=(24, 40), tgt=((96, 160),) * 3, K=200, over=3.0, imp=0.75, w_class=2.0, w_mask=5.0,
            w_dice=5.0, eos=0.1)
CASES = {
    "main": dict(BASE, seed=2941),
    "sizes": dict(BASE, seed=2702, L=2, B=2, G=(2, 3), tgt=((96, 160), (64, 128))),
    "imp0": dict(BASE, seed=2723, L=1, imp=0.0),
    "imp1": dict(BASE, seed=2744, L=1, imp=1.0),
    "q_lt_g": dict(BASE, seed=2705, L=1, B=1, G=(5,), Q=3, tgt=((96, 160),)),
}
CAPACITY = dict(BASE, seed=2706, L=1, B=1, G=(2,), Q=4, tgt=((96, 160),), K=12544)      # not in F27: its draws alone exceed a fixture's size
# Beside F27 (draws too large for a fixture), against this oracle alone; conditions 2 and 3 hold for them as for F27's cases.  The cost
# kernel works in chunks of 512 points, tiles of 64 queries and 1, 2, 4 or 8 tiles of 16 targets: F27's cases stay inside one of each.
EXTRA = {
    "capacity": CAPACITY,                                                                          # 25 chunks of points
    "wide2": dict(BASE, seed=3115, L=1, B=2, G=(20, 9), Q=70, K=600, tgt=((96, 160),) * 2),        # 2 chunks, 2 query tiles, 2 target tiles (1 used by image 1)
    "wide4": dict(BASE, seed=3200, L=1, B=1, G=(40,), Q=70, K=600, tgt=((96, 160),)),              # 4 target tiles
    "wide8": dict(BASE, seed=3320, L=1, B=1, G=(66,), Q=70, K=600, tgt=((96, 160),)),              # 8 target tiles
    "empty_big": dict(BASE, seed=3400, L=1, B=2, G=(2, 0), tgt=((64, 128), (96, 160))),            # the image without targets has the largest masks
}


def counts(case):
    """(K, oversampled, uncertain, random) with the reference's roundings."""
    K = int(case["K"])
    ku = int(case["imp"] * K)
    return K, int(K * case["over"]), ku, K - ku


def pairs_per_layer(case):
    return sum(min(case["Q"], g) for g in case["G"])


# ---------------------------------------------------------------------------------------------------
# the planted scenario
# ---------------------------------------------------------------------------------------------------
def _blob(rng, H, W):
    y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
    h, w = int(rng.integers(H // 4, H // 2)), int(rng.integers(W // 4, W // 2))
    m = np.zeros((H, W), np.float32)
    m[y0:y0 + h, x0:x0 + w] = 1.0
    return m


def _down(mask, h, w):
    """Block mean of a mask to h x w (sizes divide, or the mask is cropped to a multiple first)."""
    H, W = mask.shape
    fy, fx = H // h, W // w
    return mask[:fy * h, :fx * w].reshape(h, fy, w, fx).mean((1, 3))


def scenario(case):
    """(layers, targets) as numpy: layers[l] = (pred_logits [B, Q, C + 1], pred_masks [B, Q, h, w]) fp32; targets[b] = (labels int64 [G],
    masks uint8 [G, H, W]).  Planted per image with targets: query 0 follows target 0 almost exactly (amplitudes up to 30, so softplus
    and the sigmoid saturate), queries 1 and 2 compete for target 1, no query resembles target 2, and the LAST target's mask is all
    zero; the amplitude of every plane varies from pixel to pixel, so |x| has no plateaus the point selection could tie on."""
    rng = np.random.default_rng(case["seed"])
    h, w = case["pred"]
    targets = []
    for b in range(case["B"]):
        g, (H, W) = case["G"][b], case["tgt"][b]
        masks = np.stack([_blob(rng, H, W) for _ in range(g)]) if g else np.zeros((0, H, W), np.float32)
        if g >= 3:
            masks[g - 1] = 0.0
        targets.append((rng.integers(0, case["C"], g).astype(np.int64), masks.astype(np.uint8)))
    layers = []
    for l in range(case["L"]):
        logits = (rng.standard_normal((case["B"], case["Q"], case["C"] + 1)) * 3.0).astype(np.float32)
        masks = np.empty((case["B"], case["Q"], h, w), np.float32)
        for b in range(case["B"]):
            g = case["G"][b]
            for q in range(case["Q"]):
                amp = rng.uniform(2.0, 9.0, (h, w))
                plane = rng.standard_normal((h, w)) * amp - 4.0
                follow = {0: 0, 1: 1, 2: 1}.get(q)
                if follow is not None and follow < g and g > 1:
                    sign = 2.0 * _down(targets[b][1][follow].astype(np.float64), h, w) - 1.0
                    strength = (rng.uniform(12.0, 30.0, (h, w)), rng.uniform(3.0, 6.0 + l, (h, w)), rng.uniform(1.0, 4.0 + 2 * l, (h, w)))[q]
                    plane = sign * strength + (0.0 if q == 0 else 0.3) * plane
                    logits[b, q, targets[b][0][follow]] += (8.0, 3.0, 2.0)[q]
                masks[b, q] = plane
        layers.append((logits, masks.astype(np.float32)))
    return layers, targets


def _border_points(n, sizes):
    """Points within half a pixel of every border and corner of the finest plane, and of the coarsest."""
    out = []
    for H, W in sizes:
        ex, ey = 0.25 / W, 0.25 / H
        out += [(ex, 0.37), (1 - ex, 0.61), (0.43, ey), (0.58, 1 - ey), (ex, ey), (1 - ex, 1 - ey), (ex, 1 - ey), (1 - ex, ey)]
    return np.asarray(out[:n], np.float32)


def draws(case):
    """The planted ``torch.rand`` draws of one forward, in the reference's order: a list of fp32 arrays in [0, 1)."""
    rng = np.random.default_rng(case["seed"] + 100000)
    K, KO, KU, KR = counts(case)
    N = pairs_per_layer(case)
    sizes = [max(case["tgt"]), case["pred"]]
    out = []

    def draw(*shape):
        a = rng.random(shape, dtype=np.float32)
        a = np.minimum(a, np.float32(1.0 - 2.0 ** -24))
        edge = _border_points(shape[1], sizes)
        a[:, :len(edge)] = edge
        return a

    for _ in range(case["L"]):
        out += [draw(1, K, 2) for _ in range(case["B"])]
        out.append(draw(N, KO, 2))
        if KR > 0:
            out.append(draw(N, KR, 2))
    return out


class Queue:
    """``rand=`` of the native classes (and the stand-in for ``torch.rand`` under the reference): the planted draws in order."""

    def __init__(self, arrays, dtype=torch.float32):
        self.arrays, self.dtype, self.at, self.shapes = list(arrays), dtype, 0, []

    def __call__(self, shape, device=None):
        a = self.arrays[self.at]
        self.at += 1
        self.shapes.append(tuple(shape))
        assert tuple(a.shape) == tuple(shape), (self.at - 1, a.shape, tuple(shape))
        return torch.from_numpy(a).to(device=device or "cpu", dtype=self.dtype)

    def done(self):
        return self.at == len(self.arrays)


def checksum(case):
    layers, targets = scenario(case)
    return np.asarray([sum(float(np.abs(a).sum(dtype=np.float64)) for a in lay) for lay in layers]
                      + [float(m.sum(dtype=np.float64)) + float(lab.sum()) for lab, m in targets])


def tensors(case, dtype, device="cpu", grad=False):
    """The scenario as the modules take it: (outputs dict with aux_outputs, targets list of dicts, leaf tensors per layer)."""
    layers, targets = scenario(case)
    leaves = [(torch.tensor(lg, dtype=dtype, device=device, requires_grad=grad), torch.tensor(mk, dtype=dtype, device=device, requires_grad=grad))
              for lg, mk in layers]
    dicts = [{"pred_logits": lg, "pred_masks": mk} for lg, mk in leaves]
    outputs = dict(dicts[0])
    if len(dicts) > 1:
        outputs["aux_outputs"] = dicts[1:]
    tg = [{"labels": torch.tensor(lab, device=device), "masks": torch.tensor(m, device=device)} for lab, m in targets]
    return outputs, tg, leaves


# ---------------------------------------------------------------------------------------------------
# the reference's operators
# ---------------------------------------------------------------------------------------------------
def point_sample(inp, coords):
    """detectron2's point_sample: inp [N, C, H, W] at coords [N, P, 2] in [0, 1] (x first) -> [N, C, P]."""
    return F.grid_sample(inp, 2.0 * coords.unsqueeze(2) - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(3)


def batch_dice_loss(inputs, targets):
    inputs = inputs.sigmoid().flatten(1)
    numerator = 2 * torch.einsum("nc,mc->nm", inputs, targets)
    denominator = inputs.sum(-1)[:, None] + targets.sum(-1)[None, :]
    return 1 - (numerator + 1) / (denominator + 1)


def batch_sigmoid_ce_loss(inputs, targets):
    hw = inputs.shape[1]
    pos = F.binary_cross_entropy_with_logits(inputs, torch.ones_like(inputs), reduction="none")
    neg = F.binary_cross_entropy_with_logits(inputs, torch.zeros_like(inputs), reduction="none")
    return (torch.einsum("nc,mc->nm", pos, targets) + torch.einsum("nc,mc->nm", neg, (1 - targets))) / hw


def dice_loss(inputs, targets, num_masks):
    inputs = inputs.sigmoid().flatten(1)
    numerator = 2 * (inputs * targets).sum(-1)
    denominator = inputs.sum(-1) + targets.sum(-1)
    return (1 - (numerator + 1) / (denominator + 1)).sum() / num_masks


def sigmoid_ce_loss(inputs, targets, num_masks):
    return F.binary_cross_entropy_with_logits(inputs, targets, reduction="none").mean(1).sum() / num_masks


def nested(masks):
    """nested_tensor_from_tensor_list of [G_b, H_b, W_b] masks: zero-padded at the bottom and right to the batch's largest size."""
    H, W = max(m.shape[1] for m in masks), max(m.shape[2] for m in masks)
    return [F.pad(m, (0, W - m.shape[2], 0, H - m.shape[1])) for m in masks]


def cost_matrices(case, layer, targets, rand):
    """HungarianMatcher.memory_efficient_forward up to the cost matrices: [Q, G_b] per image (one draw each)."""
    out = []
    for b in range(len(targets)):
        prob = layer["pred_logits"][b].softmax(-1)
        cost_class = -prob[:, targets[b]["labels"].long()]
        out_mask = layer["pred_masks"][b][:, None]
        tgt_mask = targets[b]["masks"].to(out_mask)[:, None]
        pts = rand((1, case["K"], 2), out_mask.device).to(out_mask)
        tgt = point_sample(tgt_mask, pts.repeat(tgt_mask.shape[0], 1, 1)).squeeze(1)
        src = point_sample(out_mask, pts.repeat(out_mask.shape[0], 1, 1)).squeeze(1)
        C = case["w_mask"] * batch_sigmoid_ce_loss(src, tgt) + case["w_class"] * cost_class + case["w_dice"] * batch_dice_loss(src, tgt)
        out.append(C.reshape(layer["pred_logits"].shape[1], -1))
    return out


def assign(costs):
    out = []
    for C in costs:
        i, j = linear_sum_assignment(C.detach().cpu().numpy())
        out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
    return out


def run(case, dtype=torch.float64, queue=None, chosen=None, indices=None, grad=False, device="cpu"):
    """The whole criterion on the scenario.  ``chosen`` (per layer [N, KU] indices into the oversampled points) and ``indices`` (per layer,
    per image) teacher-force the point selection and the matching.  Returns a dict: costs[l][b], indices[l][b], x_over[l] [N, KO] (the
    sampled values the selection ranks), chosen[l], losses [L, 3] (ce, mask, dice), leaves (for .grad after a backward), num_masks."""
    outputs, targets, leaves = tensors(case, dtype, device, grad)
    layers = [{k: v for k, v in outputs.items() if k != "aux_outputs"}] + list(outputs.get("aux_outputs", ()))
    rand = queue or Queue(draws(case), dtype)
    K, KO, KU, KR = counts(case)
    num_masks = max(float(sum(case["G"])), 1.0)
    weight = torch.ones(case["C"] + 1)                         # the reference's buffer: made in fp32, then cast with the module
    weight[-1] = case["eos"]
    weight = weight.to(device=device, dtype=dtype)
    padded = nested([t["masks"] for t in targets])
    res = dict(costs=[], indices=[], x_over=[], chosen=[], losses=[], leaves=leaves, num_masks=num_masks)
    for l, layer in enumerate(layers):
        with torch.no_grad():
            costs = cost_matrices(case, layer, targets, rand)
        idx = indices[l] if indices is not None else assign(costs)
        res["costs"].append(costs)
        res["indices"].append(idx)
        # loss_labels
        logits = layer["pred_logits"]
        classes = torch.full(logits.shape[:2], case["C"], dtype=torch.int64, device=device)
        for b, (src, tgt) in enumerate(idx):
            classes[b, src] = targets[b]["labels"][tgt].long()
        loss_ce = F.cross_entropy(logits.transpose(1, 2), classes, weight)
        # loss_masks
        batch_idx = torch.cat([torch.full_like(src, b) for b, (src, _) in enumerate(idx)])
        src_idx = torch.cat([src for src, _ in idx])
        src_masks = layer["pred_masks"][batch_idx, src_idx][:, None]
        tgt_masks = torch.cat([padded[b][tgt] for b, (_, tgt) in enumerate(idx)]).to(src_masks)[:, None]
        N = src_masks.shape[0]
        with torch.no_grad():
            over = rand((N, KO, 2), device).to(src_masks)
            x_over = point_sample(src_masks, over)[:, 0]
            pick = chosen[l].to(device) if chosen is not None else torch.topk(-x_over.abs(), k=KU, dim=1)[1]
            coords = torch.gather(over, 1, pick[:, :, None].expand(N, KU, 2))
            if KR > 0:
                coords = torch.cat([coords, rand((N, KR, 2), device).to(src_masks)], 1)
            labels = point_sample(tgt_masks, coords).squeeze(1)
        point_logits = point_sample(src_masks, coords).squeeze(1)
        res["x_over"].append(x_over)
        res["chosen"].append(pick)
        res["losses"].append(torch.stack([loss_ce, sigmoid_ce_loss(point_logits, labels, num_masks), dice_loss(point_logits, labels, num_masks)]))
    res["losses"] = torch.stack(res["losses"])
    return res


def loss_names(L, name=None):
    """The keys of the criterion's dict in the order of ``losses [L, 3]``."""
    out = []
    for l in range(L):
        s = "" if l == 0 else f"_{l - 1}"
        out.append(tuple((f"{name}_" if name else "") + k + s for k in ("loss_ce", "loss_mask", "loss_dice")))
    return out


# ---------------------------------------------------------------------------------------------------
# the conditions on the scenario
# ---------------------------------------------------------------------------------------------------
def assignment_margin(C):
    """How much dearer the best assignment becomes when any one of its pairs is forbidden, over the largest |cost| (inf without pairs)."""
    C = np.asarray(C, np.float64)
    if C.size == 0:
        return float("inf")
    i, j = linear_sum_assignment(C)
    best, worst = C[i, j].sum(), float("inf")
    big = np.abs(C).sum() + 1.0
    for a, b in zip(i, j):
        D = C.copy()
        D[a, b] = big
        ii, jj = linear_sum_assignment(D)
        worst = min(worst, D[ii, jj].sum() - best)
    return worst / np.abs(C).max()


def undecided(x64, x32, ku):
    """Per pair the boolean mask [N, KO] of points whose |x| lies within 4 x the fp32 floor of the sampled values of the ku-th smallest."""
    x64 = x64.double().cpu()
    if ku == 0 or x64.numel() == 0:
        return torch.zeros_like(x64, dtype=torch.bool)
    floor = torch.maximum((x32.double().cpu() - x64).abs().amax(1), EPS32 * x64.abs().amax(1))
    kth = x64.abs().sort(1).values[:, ku - 1]
    return (x64.abs() - kth[:, None]).abs() <= 4.0 * floor[:, None]


def differs_only_in(a, b, mask):
    """Whether the index sets a and b ([N, KU]) differ only in points of ``mask`` ([N, KO])."""
    for n in range(a.shape[0]):
        sa, sb = set(a[n].tolist()), set(b[n].tolist())
        if len(sa) != a.shape[1] or len(sb) != b.shape[1]:
            return False
        if any(not bool(mask[n, i]) for i in sa ^ sb):
            return False
    return True
