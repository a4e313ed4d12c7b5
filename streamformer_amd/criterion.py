"""Native Mask2Former criterion: ``HungarianMatcher`` and ``SetCriterion`` of the reference's ``mask2former/modeling/matcher.py`` and
``criterion.py`` on the ``sf_op_crit_*`` kernels (csrc/sf_criterion.hip).

One training step, all decoder layers (the final one and ``aux_outputs``) at once:

1. every ``torch.rand`` draw of the reference, in the reference's order (per layer: one ``[1, num_points, 2]`` draw per image for the
   matcher, then ``[N, int(num_points * oversample_ratio), 2]`` and, when ``num_points - int(importance_sample_ratio * num_points) > 0``,
   ``[N, that, 2]`` for the mask losses; N, the layer's matched pairs, is ``sum(min(Q, G_b))`` and known before matching);
2. ``sf_op_crit_costs``: every cost matrix ``[L, B, Q, G_max]`` in one call;
3. ONE device-to-host copy (``_device_to_host``) and ``scipy.optimize.linear_sum_assignment`` per (layer, image) on the host;
4. ``sf_op_crit_class_loss`` and ``sf_op_crit_losses`` for the matched pairs of all layers, behind one ``torch.autograd.Function`` whose
   backward is ``sf_op_crit_losses_backward`` and the class gradient the forward already wrote.

``rand=None`` of both classes is a callable ``(shape, device) -> tensor in [0, 1)`` that replaces the ``torch.rand`` draws (tests and
fixtures pin the points with it); the default draws on the device.  ``SetCriterion.matcher`` may be any module that returns the
reference's indices (the reference's own matcher): it is then called once per layer, in the reference's order, and only the losses run
natively.  There is no CPU fallback.  Chosen points: the ``int(importance_sample_ratio * num_points)`` oversampled points of smallest
``|x|``, ties at the threshold to the lower index (``torch.topk`` leaves that open), in index order.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as nat

__all__ = ["HungarianMatcher", "SetCriterion"]

LOSSES = ("labels", "masks")
MAX_LAYERS, MAX_IMAGES, MAX_TARGETS = 16, 32, 128
Indices = List[Tuple[torch.Tensor, torch.Tensor]]


def _device_to_host(buffer: torch.Tensor) -> torch.Tensor:
    """The step's single device-to-host copy: the cost matrices into pinned memory, then one synchronisation of the stream."""
    host = torch.empty(buffer.shape, dtype=buffer.dtype, pin_memory=True)
    host.copy_(buffer, non_blocking=True)
    torch.cuda.current_stream(buffer.device).synchronize()
    return host


def _default_rand(shape, device) -> torch.Tensor:
    return torch.rand(shape, device=device)


def _draw(rand: Optional[Callable], shape, device) -> torch.Tensor:
    t = (rand or _default_rand)(tuple(shape), device)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"rand returned {tuple(t.shape)} for a draw of {tuple(shape)}")
    return t.to(device=device, dtype=torch.float32)


def _summary(kind: str, module: nn.Module, names: Sequence[str], indent: int, first: Optional[Tuple[str, str]] = None) -> str:
    """The text the reference's ``__repr__`` gives: ``<kind> <class>``, then one indented ``name: value`` line per attribute."""
    fields = ([first] if first else []) + [(n, getattr(module, n)) for n in names]
    return "\n".join([f"{kind} {type(module).__name__}"] + [f"{' ' * indent}{n}: {v}" for n, v in fields])


def _layers_of(outputs: Dict[str, Any]) -> List[Dict[str, Any]]:
    return [{k: v for k, v in outputs.items() if k != "aux_outputs"}] + list(outputs.get("aux_outputs", ()))


def _num_masks(targets: Sequence[Dict[str, Any]], device) -> float:
    """The reference's normaliser: the sum of ``len(labels)``, averaged over the ranks when torch.distributed runs, at least 1."""
    n = float(sum(len(t["labels"]) for t in targets))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        t = torch.as_tensor([n], dtype=torch.float, device=device)
        torch.distributed.all_reduce(t)
        n = float(t.item()) / torch.distributed.get_world_size()
    return max(n, 1.0)


class _Batch:
    """What the entry points take of one step: the layers' tensors (fp32, contiguous, one shape), the targets (masks as fp32, labels as
    int64, on the device) and their host tables.  Every refusal that needs no launch is made here."""

    def __init__(self, layers: Sequence[Dict[str, Any]], targets: Sequence[Dict[str, Any]], who: str):
        if not layers:
            raise ValueError(f"{who}: no layer")
        tensors = [t for l in layers for t in (l["pred_logits"], l["pred_masks"])] + [t[k] for t in targets for k in ("labels", "masks")]
        for t in tensors:
            if t.device.type != "cuda":
                raise RuntimeError(f"{who} runs on the MI355X: CPU tensors are refused, move outputs and targets with .to('cuda') (there is no CPU fallback)")
        self.device = layers[0]["pred_logits"].device
        self.logits = [l["pred_logits"].float().contiguous() for l in layers]
        self.masks = [l["pred_masks"].float().contiguous() for l in layers]
        if self.logits[0].dim() != 3 or self.masks[0].dim() != 4:
            raise ValueError(f"{who}: pred_logits [B, Q, C + 1] and pred_masks [B, Q, H, W], got {tuple(self.logits[0].shape)} and {tuple(self.masks[0].shape)}")
        self.L = len(layers)
        self.B, self.Q, self.C1 = self.logits[0].shape
        self.H, self.W = self.masks[0].shape[2:]
        for lg, mk in zip(self.logits, self.masks):
            if tuple(lg.shape) != (self.B, self.Q, self.C1) or tuple(mk.shape) != (self.B, self.Q, self.H, self.W):
                raise ValueError(f"{who}: every layer must have the final layer's shapes, got {tuple(lg.shape)} and {tuple(mk.shape)}")
        if len(targets) != self.B:
            raise ValueError(f"{who}: {len(targets)} targets for a batch of {self.B}")
        self.tgt_masks = [t["masks"].to(torch.float32).contiguous() for t in targets]
        self.tgt_labels = [t["labels"].to(torch.int64).contiguous() for t in targets]
        self.G = [int(t.shape[0]) for t in self.tgt_labels]
        for b, m in enumerate(self.tgt_masks):
            if m.dim() != 3 or m.shape[0] != self.G[b]:
                raise ValueError(f"{who}: image {b}: masks {tuple(m.shape)} for {self.G[b]} labels")
        if self.L > MAX_LAYERS or self.B > MAX_IMAGES or max(self.G, default=0) > MAX_TARGETS:
            raise RuntimeError(f"{who}: capacity limit: {self.L} layers (up to {MAX_LAYERS}), {self.B} images (up to {MAX_IMAGES}), "
                               f"{max(self.G, default=0)} targets in an image (up to {MAX_TARGETS})")
        self.G_max = max(max(self.G, default=0), 1)
        self.c_logits, self.c_masks = nat.ptr_array(self.logits), nat.ptr_array(self.masks)
        self.c_tgt_masks, self.c_tgt_labels = nat.ptr_array(self.tgt_masks), nat.ptr_array(self.tgt_labels)
        self.c_G = nat.i32_array(self.G)
        self.c_H, self.c_W = nat.i32_array([m.shape[1] for m in self.tgt_masks]), nat.i32_array([m.shape[2] for m in self.tgt_masks])

    def pairs_expected(self) -> int:
        return sum(min(self.Q, g) for g in self.G)


def _cost_matrices(batch: _Batch, coords: torch.Tensor, K: int, w_class: float, w_mask: float, w_dice: float, cost: Optional[torch.Tensor] = None):
    """``sf_op_crit_costs``: cost [L, B, Q, G_max] on the device (columns >= G_b unwritten)."""
    if cost is None:
        cost = torch.zeros(batch.L, batch.B, batch.Q, batch.G_max, dtype=torch.float32, device=batch.device)
    coords = coords.to(torch.float32).contiguous()
    if tuple(coords.shape) != (batch.L, batch.B, K, 2):
        raise ValueError(f"point coordinates {tuple(coords.shape)} are not [L, B, K, 2] = {(batch.L, batch.B, K, 2)}")
    nat.launch(batch.device, nat.lib.sf_op_crit_costs, batch.c_logits, batch.c_masks, batch.L, batch.B, batch.Q, batch.C1, batch.H, batch.W,
               batch.c_tgt_masks, batch.c_tgt_labels, batch.c_G, batch.c_H, batch.c_W, coords.data_ptr(), K, batch.G_max, float(w_class),
               float(w_mask), float(w_dice), cost.data_ptr(),
               workspace=nat.scratch(nat.lib.sf_op_crit_costs_workspace_bytes(batch.L, batch.B, batch.Q, batch.G_max, K), batch.device))
    return cost


def assign(cost_host: np.ndarray, G: Sequence[int]) -> List[Indices]:
    """The host step: ``linear_sum_assignment`` of cost_host [L, B, Q, >= G_b] per (layer, image), the reference's solver."""
    out = []
    for l in range(cost_host.shape[0]):
        layer = []
        for b, g in enumerate(G):
            i, j = linear_sum_assignment(cost_host[l, b, :, :g]) if g else (np.zeros(0, np.int64), np.zeros(0, np.int64))
            layer.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        out.append(layer)
    return out


class HungarianMatcher(nn.Module):
    """The reference's matcher.  ``forward(outputs, targets)`` returns ``[(index_i, index_j)]`` int64 CPU tensors per image, in the order
    ``scipy.optimize.linear_sum_assignment`` gives; ``match_layers`` does the same for several layers with one launch and one copy."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0, rand: Optional[Callable] = None):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        if cost_class == 0 and cost_mask == 0 and cost_dice == 0:      # the reference's refusal, an AssertionError there as well
            raise AssertionError("HungarianMatcher: cost_class, cost_mask and cost_dice are all 0, so every assignment would cost the same")
        self.num_points = num_points
        self.rand = rand

    def draw_points(self, images: int, device) -> torch.Tensor:
        """One layer's draws, one ``[1, num_points, 2]`` per image as the reference makes them: [B, K, 2]."""
        return torch.cat([_draw(self.rand, (1, self.num_points, 2), device) for _ in range(images)])

    @torch.no_grad()
    def match_layers(self, layers: Sequence[Dict[str, Any]], targets: Sequence[Dict[str, Any]], coords: Optional[torch.Tensor] = None,
                     batch: Optional[_Batch] = None) -> List[Indices]:
        if self.num_points < 1:
            raise ValueError("HungarianMatcher: num_points must be at least 1")
        batch = batch or _Batch(layers, targets, "HungarianMatcher")
        if coords is None:
            coords = torch.stack([self.draw_points(batch.B, batch.device) for _ in range(batch.L)])
        if max(batch.G, default=0) == 0:                       # no target anywhere: nothing to launch, nothing to copy
            return assign(np.zeros((batch.L, batch.B, batch.Q, 0), np.float32), batch.G)
        cost = _cost_matrices(batch, coords, self.num_points, self.cost_class, self.cost_mask, self.cost_dice)
        return assign(_device_to_host(cost).numpy(), batch.G)

    @torch.no_grad()
    def memory_efficient_forward(self, outputs, targets) -> Indices:
        return self.match_layers([outputs], targets)[0]

    @torch.no_grad()
    def forward(self, outputs, targets) -> Indices:
        return self.memory_efficient_forward(outputs, targets)

    def __repr__(self, _repr_indent=4):      # the keyword is how the reference's criterion asks for a deeper indent
        return _summary("Matcher", self, ("cost_class", "cost_mask", "cost_dice"), _repr_indent)


def pair_table(indices: Sequence[Indices]) -> Tuple[np.ndarray, List[int]]:
    """(pairs int32 [N, 4] of (layer, image, query, target), layer_start [L + 1]) of per-layer indices, in layer, image and match order:
    the order of the reference's ``_get_src_permutation_idx``."""
    rows, start = [], [0]
    for l, layer in enumerate(indices):
        for b, (src, tgt) in enumerate(layer):
            src, tgt = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(tgt, dtype=np.int64).reshape(-1)
            if src.shape != tgt.shape:
                raise ValueError(f"layer {l}, image {b}: {src.size} query indices for {tgt.size} target indices")
            rows.append(np.stack([np.full_like(src, l), np.full_like(src, b), src, tgt], 1))
        start.append(sum(len(r) for r in rows))
    pairs = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)
    return np.ascontiguousarray(pairs), start


def _check_pairs(pairs: np.ndarray, batch: _Batch) -> None:
    for b, g in enumerate(batch.G):
        sel = pairs[pairs[:, 1] == b]
        if sel.size and (sel[:, 2].min() < 0 or sel[:, 2].max() >= batch.Q or sel[:, 3].min() < 0 or sel[:, 3].max() >= g):
            raise ValueError(f"image {b}: matched indices outside {batch.Q} queries / {g} targets")


class _Step:
    """One step's native calls and what its backward needs."""

    def __init__(self, batch: _Batch, pairs: np.ndarray, layer_start: List[int], num_masks: float, want_labels: bool, want_masks: bool,
                 empty_weight: Optional[torch.Tensor], K: int, K_over: int, K_uncertain: int, over: Optional[torch.Tensor], rnd: Optional[torch.Tensor],
                 debug: bool = False):
        self.batch, self.num_masks, self.want_labels, self.want_masks = batch, float(num_masks), want_labels, want_masks
        self.K, self.K_over, self.K_uncertain = K, K_over, K_uncertain
        self.N = int(pairs.shape[0])
        _check_pairs(pairs, batch)
        dev = batch.device
        self.pairs = torch.from_numpy(pairs).to(dev, non_blocking=True) if self.N else torch.zeros(1, 4, dtype=torch.int32, device=dev)
        self.c_start = nat.i32_array(layer_start)
        self.empty_weight, self.over, self.rnd = empty_weight, over, rnd
        self.class_grad = self.coords = self.sums = self.chosen = self.target_classes = None
        self.debug = debug                                     # tests: keep the draws and write the chosen indices

    def forward(self, need_grad: bool = True) -> torch.Tensor:
        b, dev = self.batch, self.batch.device
        out = torch.zeros(b.L, 3, dtype=torch.float32, device=dev)
        if self.want_labels:
            w = self.empty_weight.to(device=dev, dtype=torch.float32).contiguous()
            if w.numel() != b.C1:
                raise ValueError(f"empty_weight has {w.numel()} entries for {b.C1} class logits")
            self.class_grad = torch.empty(b.L, b.B, b.Q, b.C1, dtype=torch.float32, device=dev) if need_grad else None
            self.target_classes = torch.empty(b.L, b.B, b.Q, dtype=torch.int32, device=dev)
            nat.launch(dev, nat.lib.sf_op_crit_class_loss, b.c_logits, b.L, b.B, b.Q, b.C1, self.pairs.data_ptr(), self.N, b.c_tgt_labels, b.c_G,
                       w.data_ptr(), out.data_ptr(), 3, nat.ptr(self.class_grad), self.target_classes.data_ptr(),
                       workspace=nat.scratch(nat.lib.sf_op_crit_class_loss_workspace_bytes(b.L, b.B, b.Q), dev))
        if self.want_masks:
            n = max(self.N, 1)
            self.coords = torch.zeros(n, self.K, 2, dtype=torch.float32, device=dev)
            self.sums = torch.zeros(n, 4, dtype=torch.float32, device=dev)
            self.chosen = torch.zeros(n, max(self.K_uncertain, 1), dtype=torch.int32, device=dev) if self.debug else None
            nat.launch(dev, nat.lib.sf_op_crit_losses, b.c_masks, b.L, b.B, b.Q, b.H, b.W, b.c_tgt_masks, b.c_G, b.c_H, b.c_W, self.pairs.data_ptr(),
                       self.c_start, self.N, nat.ptr(self.over), nat.ptr(self.rnd), self.K, self.K_over, self.K_uncertain, self.num_masks,
                       out[:, 1:].data_ptr(), 3, self.coords.data_ptr(), self.sums.data_ptr(), nat.ptr(self.chosen),
                       workspace=nat.scratch(nat.lib.sf_op_crit_losses_workspace_bytes(self.N), dev))
        return out

    def backward_masks(self, upstream: torch.Tensor) -> torch.Tensor:
        """grad_pred_masks [L, B, Q, H, W] for upstream [L, 2] = d / d (loss_mask_l, loss_dice_l)."""
        b, dev = self.batch, self.batch.device
        grad = torch.empty(b.L, b.B, b.Q, b.H, b.W, dtype=torch.float32, device=dev)
        upstream = upstream.to(torch.float32).contiguous()
        nat.launch(dev, nat.lib.sf_op_crit_losses_backward, b.c_masks, b.L, b.B, b.Q, b.H, b.W, b.c_tgt_masks, b.c_G, b.c_H, b.c_W, self.pairs.data_ptr(),
                   self.N, self.coords.data_ptr(), self.sums.data_ptr(), self.K, self.num_masks, upstream.data_ptr(), grad.data_ptr())
        return grad


class _CriterionFunction(Function):
    """losses [L, 3] = (loss_ce, loss_mask, loss_dice) per layer of the layers' pred_logits and pred_masks (``tensors``: L + L)."""

    @staticmethod
    def forward(ctx, step: _Step, *tensors):
        ctx.step = step
        ctx.save_for_backward(*tensors[step.batch.L:])         # backward samples pred_masks again: autograd then sees a change in place
        out = step.forward(need_grad=any(t.requires_grad for t in tensors))
        if not step.debug:
            step.over = step.rnd = None                        # the draws are not needed again
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        step, L = ctx.step, ctx.step.batch.L
        ctx.saved_tensors                                      # raises if a layer's pred_masks changed in place since the forward
        g_logits: List[Optional[torch.Tensor]] = [None] * L
        g_masks: List[Optional[torch.Tensor]] = [None] * L
        if step.want_labels and any(ctx.needs_input_grad[1:1 + L]):
            g = step.class_grad * grad[:, 0].reshape(L, 1, 1, 1)
            g_logits = [g[l] for l in range(L)]
        if step.want_masks and any(ctx.needs_input_grad[1 + L:]):
            g = step.backward_masks(grad[:, 1:3])
            g_masks = [g[l] for l in range(L)]
        return (None, *g_logits, *g_masks)


class SetCriterion(nn.Module):
    """The reference's criterion on the native kernels; see the module docstring.  ``forward(outputs, targets, name=None)`` returns the
    reference's dict of scalar losses, differentiable in every layer's ``pred_logits`` and ``pred_masks``."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio, importance_sample_ratio,
                 rand: Optional[Callable] = None):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.num_points = num_points
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        self.rand = rand
        self._trace: Optional[List[_Step]] = None              # tests set a list: every forward then appends its _Step, built with debug=True

    def point_counts(self) -> Tuple[int, int, int]:
        """(num_points, oversampled, uncertain) with the reference's roundings."""
        return int(self.num_points), int(self.num_points * self.oversample_ratio), int(self.importance_sample_ratio * self.num_points)

    def _check(self) -> None:
        for loss in self.losses:
            if loss not in LOSSES:
                raise ValueError(f"SetCriterion: do you really want to compute {loss} loss?  The native criterion has {LOSSES}")
        if "masks" in self.losses:
            if self.oversample_ratio < 1:
                raise ValueError(f"SetCriterion: oversample_ratio = {self.oversample_ratio} must be at least 1")
            if not 0 <= self.importance_sample_ratio <= 1:
                raise ValueError(f"SetCriterion: importance_sample_ratio = {self.importance_sample_ratio} must lie in [0, 1]")
            K, K_over, _ = self.point_counts()
            if K < 1:
                raise ValueError(f"SetCriterion: num_points = {self.num_points} must be at least 1")
            cap = nat.lib.sf_op_crit_losses_capacity()
            if K_over > cap:
                raise RuntimeError(f"SetCriterion: capacity limit: {K_over} oversampled points per pair exceed {cap} (a pair's values stay in the CU's LDS)")

    def forward(self, outputs, targets, name=None):
        self._check()
        layers = _layers_of(outputs)
        batch = _Batch(layers, targets, "SetCriterion")
        dev = batch.device
        want_labels, want_masks = "labels" in self.losses, "masks" in self.losses
        K, K_over, K_unc = self.point_counts() if want_masks else (1, 0, 0)
        native = isinstance(self.matcher, HungarianMatcher)
        over, rnd, match_points, indices = [], [], [], []
        for l, layer in enumerate(layers):                     # the reference's order: a layer's matching, then its losses
            if native:
                match_points.append(self.matcher.draw_points(batch.B, dev))
                n = batch.pairs_expected()
            else:
                indices.append(self.matcher(layer, targets))
                n = sum(len(src) for src, _ in indices[-1])
            if want_masks:
                over.append(_draw(self.rand, (n, K_over, 2), dev))
                if K - K_unc > 0:
                    rnd.append(_draw(self.rand, (n, K - K_unc, 2), dev))
        if native:
            indices = self.matcher.match_layers(layers, targets, coords=torch.stack(match_points), batch=batch)
        num_masks = _num_masks(targets, dev)
        pairs, start = pair_table(indices)
        step = _Step(batch, pairs, start, num_masks, want_labels, want_masks, self.empty_weight, K, K_over, K_unc,
                     torch.cat(over).contiguous() if over else None, torch.cat(rnd).contiguous() if rnd else None, debug=self._trace is not None)
        if self._trace is not None:
            self._trace.append(step)
        out = _CriterionFunction.apply(step, *[l["pred_logits"] for l in layers], *[l["pred_masks"] for l in layers])
        losses = {}
        for l in range(batch.L):
            suffix = "" if l == 0 else f"_{l - 1}"
            for loss in self.losses:
                if loss == "labels":
                    losses["loss_ce" + suffix] = out[l, 0]
                else:
                    losses["loss_mask" + suffix] = out[l, 1]
                    losses["loss_dice" + suffix] = out[l, 2]
        if name is not None:
            return {f"{name}_{k}": v for k, v in losses.items()}
        return losses

    def __repr__(self):
        try:
            matcher = self.matcher.__repr__(_repr_indent=8)
        except TypeError:                                      # a foreign matcher without the reference's keyword
            matcher = repr(self.matcher)
        names = ("losses", "weight_dict", "num_classes", "eos_coef", "num_points", "oversample_ratio", "importance_sample_ratio")
        return _summary("Criterion", self, names, 4, first=("matcher", matcher))
