"""Native Mask2Former criterion against the reference's operator sequence in torch on the same GPU -> profiles/criterion.txt

    python tools/criterion_bench.py [--smoke]

Synthetic inputs at the shipped shapes, hard-coded from the reference's config: Q = 100 queries, K = 112 * 112 = 12544 points, oversample
3.0, importance 0.75, L = 10 decoder layers (DEC_LAYERS; the final one plus nine auxiliary), C = 40 classes, B = 2 frames, predicted masks
at stride 4 of a 384 x 640 training crop (96 x 160), target masks 384 x 640, (4, 6) targets.  Both sides run forward and backward of the
summed losses; medians of 10 with tools/_timing.py.  The torch side is the reference's sequence restated here with ``F.grid_sample``: per
layer and image the matcher's two samplings, two einsums per cost and ``C.cpu()``, per layer the oversampled sampling, ``topk``, the
gather and the two pair losses.  What is counted on both sides are the device-to-host copies, each of which makes the host wait for the
GPU: the native step's copy helper, the torch side's ``.cpu()`` calls.  Host-to-device uploads from pageable memory (the native step's
pair table, the torch side's index tensors) also hold the host for the length of the copy; they are not counted on either side.
"""
import os
import sys

import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamformer_amd as sa                      # noqa: E402
from streamformer_amd import criterion as K        # noqa: E402
from _timing import timed                          # noqa: E402

SHIPPED = dict(L=10, B=2, Q=100, C=40, pred=(96, 160), tgt=(384, 640), G=(4, 6), points=12544, over=3.0, imp=0.75)
SMOKE = dict(SHIPPED, L=2, Q=20, pred=(24, 40), tgt=(96, 160), points=200)
WEIGHTS = dict(w_class=2.0, w_mask=5.0, w_dice=5.0, eos=0.1)


def sample(inp, pts):
    return F.grid_sample(inp, 2.0 * pts.unsqueeze(2) - 1.0, align_corners=False).squeeze(3)


class TorchCriterion:
    """The reference's operator sequence (matcher.py, criterion.py) in torch; ``syncs`` counts its device-to-host copies."""

    def __init__(self, s):
        self.s, self.syncs = s, 0
        self.weight = torch.ones(s["C"] + 1, device="cuda")
        self.weight[-1] = WEIGHTS["eos"]

    def match(self, layer, targets):
        out = []
        for b, t in enumerate(targets):
            prob = layer["pred_logits"][b].softmax(-1)
            cost_class = -prob[:, t["labels"]]
            pts = torch.rand(1, self.s["points"], 2, device="cuda")
            tgt = sample(t["masks"].float()[:, None], pts.repeat(len(t["labels"]), 1, 1)).squeeze(1)
            src = sample(layer["pred_masks"][b][:, None], pts.repeat(self.s["Q"], 1, 1)).squeeze(1)
            pos = F.binary_cross_entropy_with_logits(src, torch.ones_like(src), reduction="none")
            neg = F.binary_cross_entropy_with_logits(src, torch.zeros_like(src), reduction="none")
            cost_mask = (torch.einsum("nc,mc->nm", pos, tgt) + torch.einsum("nc,mc->nm", neg, 1 - tgt)) / src.shape[1]
            sig = src.sigmoid()
            cost_dice = 1 - (2 * torch.einsum("nc,mc->nm", sig, tgt) + 1) / (sig.sum(-1)[:, None] + tgt.sum(-1)[None, :] + 1)
            C = WEIGHTS["w_mask"] * cost_mask + WEIGHTS["w_class"] * cost_class + WEIGHTS["w_dice"] * cost_dice
            self.syncs += 1
            i, j = linear_sum_assignment(C.cpu())
            out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        return out

    def layer_losses(self, layer, targets, num_masks):
        with torch.no_grad():
            idx = self.match(layer, targets)
        s = self.s
        classes = torch.full((s["B"], s["Q"]), s["C"], dtype=torch.int64, device="cuda")
        for b, (src, tgt) in enumerate(idx):
            classes[b, src] = targets[b]["labels"][tgt]
        loss_ce = F.cross_entropy(layer["pred_logits"].transpose(1, 2), classes, self.weight)
        batch = torch.cat([torch.full_like(src, b) for b, (src, _) in enumerate(idx)])
        src_masks = layer["pred_masks"][batch, torch.cat([src for src, _ in idx])][:, None]
        tgt_masks = torch.cat([targets[b]["masks"][tgt] for b, (_, tgt) in enumerate(idx)]).float()[:, None]
        n, ku = src_masks.shape[0], int(s["imp"] * s["points"])
        with torch.no_grad():
            over = torch.rand(n, int(s["points"] * s["over"]), 2, device="cuda")
            pick = torch.topk(-sample(src_masks, over)[:, 0].abs(), k=ku, dim=1)[1]
            pts = torch.cat([torch.gather(over, 1, pick[:, :, None].expand(n, ku, 2)), torch.rand(n, s["points"] - ku, 2, device="cuda")], 1)
            labels = sample(tgt_masks, pts).squeeze(1)
        logits = sample(src_masks, pts).squeeze(1)
        loss_mask = F.binary_cross_entropy_with_logits(logits, labels, reduction="none").mean(1).sum() / num_masks
        sig = logits.sigmoid()
        loss_dice = (1 - (2 * (sig * labels).sum(-1) + 1) / (sig.sum(-1) + labels.sum(-1) + 1)).sum() / num_masks
        return loss_ce + loss_mask + loss_dice

    def __call__(self, layers, targets):
        num_masks = float(max(sum(len(t["labels"]) for t in targets), 1))
        return sum(self.layer_losses(layer, targets, num_masks) for layer in layers)


def inputs(s):
    g = torch.Generator(device="cuda").manual_seed(0)
    layers = [{"pred_logits": torch.randn(s["B"], s["Q"], s["C"] + 1, device="cuda", generator=g).requires_grad_(),
               "pred_masks": (torch.randn(s["B"], s["Q"], *s["pred"], device="cuda", generator=g) * 4).requires_grad_()} for _ in range(s["L"])]
    targets = []
    for n in s["G"]:
        masks = torch.zeros(n, *s["tgt"], dtype=torch.bool, device="cuda")
        for i in range(n):
            masks[i, 20 * i:20 * i + s["tgt"][0] // 3, 30 * i:30 * i + s["tgt"][1] // 3] = True
        targets.append({"labels": torch.randint(0, s["C"], (n,), device="cuda", generator=g), "masks": masks})
    return layers, targets


def main():
    s = SMOKE if "--smoke" in sys.argv else SHIPPED
    layers, targets = inputs(s)
    outputs = dict(layers[0], aux_outputs=layers[1:])
    crit = sa.SetCriterion(s["C"], sa.HungarianMatcher(WEIGHTS["w_class"], WEIGHTS["w_mask"], WEIGHTS["w_dice"], s["points"]), {}, WEIGHTS["eos"],
                           ["labels", "masks"], s["points"], s["over"], s["imp"]).cuda()
    ref = TorchCriterion(s)
    copies, real = [0], K._device_to_host

    def counting(t):
        copies[0] += 1
        return real(t)
    K._device_to_host = counting

    def native():
        sum(crit(outputs, targets).values()).backward()

    def torch_side():
        ref(layers, targets).backward()

    native()
    native_syncs, copies[0] = copies[0], 0
    torch_side()
    torch_syncs = ref.syncs
    runs = 2 if "--smoke" in sys.argv else 10
    nat_ms, ref_ms = timed(native, 2, runs), timed(torch_side, 2, runs)
    ko = int(s["points"] * s["over"])
    lines = [f"Mask2Former criterion, forward + backward of the summed losses ({torch.cuda.get_device_name(0)})",
             f"shapes: L = {s['L']} layers, B = {s['B']}, Q = {s['Q']}, C = {s['C']}, masks {s['pred']}, targets {s['tgt']} x {s['G']}, K = {s['points']}, "
             f"oversample {s['over']}, importance {s['imp']}; median (min, max) ms of {runs}",
             f"native  SetCriterion            {nat_ms[0]:9.3f} ({nat_ms[1]:.3f}, {nat_ms[2]:.3f}) ms   device-to-host copies per step: {native_syncs}",
             f"torch   reference's sequence    {ref_ms[0]:9.3f} ({ref_ms[1]:.3f}, {ref_ms[2]:.3f}) ms   device-to-host copies per step: {torch_syncs}",
             f"ratio torch / native: {ref_ms[0] / nat_ms[0]:.2f}",
             f"loss kernel LDS: ({ko} + 1352) * 4 = {(ko + 1352) * 4} bytes of the CU's 163840"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if "--smoke" not in sys.argv:
        with open(os.path.join(ROOT, "profiles", "criterion.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
