"""Native CTVIS contrastive loss: ``CTCLPlugin`` of the reference's ``ctvis/modeling/cl_plugin/ct_cl_plugin.py`` on the ``sf_op_clp_*``
kernels (csrc/sf_cl_plugin.hip).  ``train_loss(det_outputs, gt_instances, matcher)`` returns the reference's dict (``loss_reid``,
``loss_aux_reid``, multiplied by ``weight_dict``, other keys dropped), differentiable in ``det_outputs["pred_embeds"]``.

One training step:

1. the matching.  With the native ``HungarianMatcher`` the reference's F per-position calls become ONE ``match_layers`` call over all
   B F images (point draws in the reference's (position, image) order, placed at image b F + f; chunks of whole frame positions when
   B F exceeds ``criterion.MAX_IMAGES``): one cost-matrix device-to-host copy.  Any other matcher is called once per position, as in
   the reference.
2. the PLAN, on the host, from the (CPU) indices and the ``valid`` flags alone: which items exist, each item's anchor row, positive
   (an embedding row or a similarity-guided embedding) and negative rows, and every instance's present / absent sequence.  The
   reference's draws are made here in its order through the hooks ``sample(population_tuple, k)`` (default ``random.sample``) and
   ``coin()`` (default ``np.random.rand``).  The plan goes to the device as one int32 table; nothing is read back.
3. ``sf_op_clp_tracks`` (similarity-guided embeddings per instance), ``sf_op_clp_items`` (per-item losses and the two sums), behind one
   ``torch.autograd.Function`` whose backward is ``sf_op_clp_backward``.

Kept quirks: the negatives of a valid instance are sampled among the FIRST ``num_negatives + 1`` queries; ``exist_after`` is the
reference's expression as written; the negatives of an item are the bank's of the frame before, all Q rows when the instance was absent
there.  ``bio_cl`` has no effect (the reference's block is commented out); ``noise_embed=True`` is refused.  There is no CPU fallback.
"""
from __future__ import annotations

import random
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as nat
from . import criterion as crit

__all__ = ["CTCLPlugin", "ctvis_train_losses"]

MAX_C = 256                      # channels of pred_embeds the kernels take: a multiple of 8 up to 256 (a lane holds 4 of a row)
MAX_F = 32                       # frames of a video: a track's frames stay in the CU's LDS
ITEM_FIELDS = 8                  # track, frame, anchor row, positive kind, positive index, first negative, negatives, positive frame
LOSS_KEYS = ("loss_reid", "loss_aux_reid")


def _default_sample(population, k):
    return random.sample(population, k)


def _default_coin():
    return np.random.rand()


class Plan:
    """The data-dependent bookkeeping of one step, decided on the host.

    ``items``       one tuple per contrastive item, in the reference's order: (video, instance, frame, anchor query, positive kind
                    (0 an embedding, 1 the similarity-guided embedding), positive frame, negative queries of frame - 1)
    ``track_rows``  int32 [T, F]: the matched row (b F + f) Q + q of a (video, instance) at every frame it is present in, else -1
    ``table``       everything the kernels read, one int32 array: track_rows [T, F], track_items [T, F] (the item of (track, frame) or
                    -1), item records [I, 8], negative rows [NE], and per destination row the items that list it as a negative
                    (row_start [R + 1], row_items [NE], in plan order)
    """

    def __init__(self, gt2query, valid, F: int, Q: int, num_negatives: int, momentum_embed: bool = True,
                 sample: Optional[Callable] = None, coin: Optional[Callable] = None):
        sample, coin = sample or _default_sample, coin or _default_coin
        nn_, B = int(num_negatives), len(valid)
        self.B, self.F, self.Q, self.R = B, F, Q, B * F * Q
        self.items: List[tuple] = []
        self.tracks = [(b, i) for b in range(B) for i in range(len(valid[b][0]) if F else 0)]
        track_of = {key: t for t, key in enumerate(self.tracks)}
        T = len(self.tracks)
        self.track_rows = np.full((T, F), -1, np.int32)
        for b in range(B):
            G = len(valid[b][0])
            present = [[bool(valid[b][f][i]) for f in range(F)] for i in range(G)]
            negs: List[List[Any]] = [[None] * F for _ in range(G)]
            for f in range(F):                                   # the bank fill: one sample per valid (frame, instance)
                taken = set()
                for i in range(G):
                    if present[i][f]:
                        q = int(gt2query[b][f][i])
                        if not 0 <= q < Q:
                            raise ValueError(f"CTCLPlugin: video {b}, frame {f}: matched query {q} outside {Q} queries")
                        if q in taken:
                            raise ValueError(f"CTCLPlugin: video {b}, frame {f}: query {q} is matched to two present instances")
                        taken.add(q)
                        self.track_rows[track_of[(b, i)], f] = (b * F + f) * Q + q
                        negs[i][f] = sorted(sample(tuple(set(range(nn_ + 1)) - set([q])), nn_))
                        if any(not 0 <= int(k) < Q for k in negs[i][f]):
                            raise ValueError(f"CTCLPlugin: sample returned a query outside {Q} queries")
                    else:
                        negs[i][f] = range(Q)
            for f in range(1, F):                                # the items, frame by frame
                for i in range(G):
                    if not present[i][f]:
                        continue
                    seq = present[i]
                    if f != sum(1 for p in seq[:f] if not p):                    # exist_before
                        if momentum_embed and coin() > 0.5:
                            kind, pf = 1, f - 1
                        else:
                            kind, pf = 0, max(j for j in range(f) if seq[j])
                    elif f != sum(1 for p in seq[f + 1:] if not p):              # exist_after, as the reference writes it
                        later = [j for j in range(f + 1, F) if seq[j]]
                        if not later:
                            continue
                        kind, pf = 0, later[0]
                    else:
                        continue
                    self.items.append((b, i, f, int(gt2query[b][f][i]), kind, pf, tuple(int(k) for k in negs[i][f - 1])))
        self.I = len(self.items)
        track_items = np.full((T, F), -1, np.int32)
        rec = np.zeros((self.I, ITEM_FIELDS), np.int32)
        neg_rows: List[int] = []
        for n, (b, i, f, q, kind, pf, neg) in enumerate(self.items):
            t = track_of[(b, i)]
            track_items[t, f] = n
            pos = t * F + pf if kind else int(self.track_rows[t, pf])
            rec[n] = (t, f, (b * F + f) * Q + q, kind, pos, len(neg_rows), len(neg), pf)
            neg_rows += [(b * F + f - 1) * Q + k for k in neg]
        self.NE = len(neg_rows)
        neg_arr = np.asarray(neg_rows, np.int32).reshape(-1)
        owner = np.repeat(np.arange(self.I, dtype=np.int32), rec[:, 6]) if self.I else np.zeros(0, np.int32)
        order = np.argsort(neg_arr, kind="stable")               # stable: a row's items stay in plan order
        row_start = np.zeros(self.R + 1, np.int32)
        np.cumsum(np.bincount(neg_arr, minlength=self.R), out=row_start[1:])
        self.max_neg = int(rec[:, 6].max()) if self.I else 0
        parts = [self.track_rows.reshape(-1), track_items.reshape(-1), rec.reshape(-1), neg_arr, row_start, owner[order]]
        self.offsets = np.cumsum([0] + [p.size for p in parts])[:-1].tolist()
        self.table = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.int32)]).astype(np.int32))
        self.T = T


class _Step:
    """One step's native calls and what its backward needs."""

    def __init__(self, plan: Plan, embeds: torch.Tensor):
        self.plan, dev = plan, embeds.device
        self.C = int(embeds.shape[-1])
        self.table = torch.from_numpy(plan.table).to(dev, non_blocking=True)
        base, o = self.table.data_ptr(), plan.offsets
        self.p_track_rows, self.p_track_items, self.p_items, self.p_neg, self.p_row_start, self.p_row_items = (base + 4 * x for x in o)
        self.sg = self.stats = self.item_out = None

    def tracks(self, e: torch.Tensor, sg: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> None:
        """sg [T, F, C] and stats [T, F, 2] = (sim, beta) of every (instance, frame)."""
        p, dev = self.plan, e.device
        self.sg = sg if sg is not None else torch.empty(max(p.T, 1), p.F, self.C, dtype=torch.float32, device=dev)
        self.stats = stats if stats is not None else torch.empty(max(p.T, 1), p.F, 2, dtype=torch.float32, device=dev)
        if p.T:
            nat.launch(dev, nat.lib.sf_op_clp_tracks, e.data_ptr(), p.R, self.C, self.p_track_rows, p.T, p.F, self.sg.data_ptr(), self.stats.data_ptr())

    def losses(self, e: torch.Tensor, out: Optional[torch.Tensor] = None, item_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(loss_reid, loss_aux_reid) [2]; item_out [I, 4] = (contras, aux, d_pos, 1 / |anchor|) per item."""
        p, dev = self.plan, e.device
        out = out if out is not None else torch.empty(2, dtype=torch.float32, device=dev)
        self.item_out = item_out if item_out is not None else torch.empty(max(p.I, 1), 4, dtype=torch.float32, device=dev)
        nat.launch(dev, nat.lib.sf_op_clp_items, e.data_ptr(), p.R, self.C, self.sg.data_ptr(), p.T, p.F, self.p_items, p.I, self.p_neg, p.NE, p.max_neg,
                   out.data_ptr(), self.item_out.data_ptr())
        return out

    def forward(self, e: torch.Tensor) -> torch.Tensor:
        self.tracks(e)
        return self.losses(e)

    def backward(self, e: torch.Tensor, upstream: torch.Tensor, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """grad_pred_embeds [R, C] for upstream [2] = d / d (loss_reid, loss_aux_reid); rows nobody references are written as zeros."""
        p, dev = self.plan, e.device
        grad = grad if grad is not None else torch.empty(p.R, self.C, dtype=torch.float32, device=dev)
        upstream = upstream.to(torch.float32).contiguous()
        nat.launch(dev, nat.lib.sf_op_clp_backward, e.data_ptr(), p.R, self.C, self.sg.data_ptr(), self.stats.data_ptr(), self.p_track_rows,
                   self.p_track_items, p.T, p.F, self.p_items, p.I, self.p_neg, p.NE, p.max_neg, self.p_row_start, self.p_row_items,
                   self.item_out.data_ptr(), upstream.data_ptr(), grad.data_ptr(),
                   workspace=nat.scratch(nat.lib.sf_op_clp_backward_workspace_bytes(p.I, p.T, p.F, self.C), dev))
        return grad


class _ReidFunction(Function):
    """(loss_reid, loss_aux_reid) [2] of pred_embeds [B F, Q, C]."""

    @staticmethod
    def forward(ctx, step: _Step, embeds):
        e = embeds.detach().float().contiguous()
        ctx.step = step
        ctx.save_for_backward(embeds, e)
        return step.forward(e)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        embeds, e = ctx.saved_tensors
        g = ctx.step.backward(e, grad)
        return None, g.view(embeds.shape).to(embeds.dtype)


def _field(target, name):
    return target[name] if isinstance(target, dict) else getattr(target, name)


class CTCLPlugin(nn.Module):
    """The reference's ``CTCLPlugin``; see the module docstring.  ``sample`` and ``coin`` replace ``random.sample`` and
    ``np.random.rand`` (tests and fixtures pin the draws with them)."""

    def __init__(self, *, weight_dict, num_negatives, sampling_frame_num, bio_cl=False, momentum_embed=True, noise_embed=False,
                 sample: Optional[Callable] = None, coin: Optional[Callable] = None):
        super().__init__()
        if noise_embed:
            raise NotImplementedError("CTCLPlugin: noise_embed=True is not supported (the reference's default and every shipped config have it off)")
        self.weight_dict = weight_dict
        self.num_negatives = num_negatives
        self.sampling_frame_num = sampling_frame_num
        self.bio_cl = bio_cl                                      # accepted, without effect: as in the reference
        self.momentum_embed = momentum_embed
        self.noise_embed = noise_embed
        self.sample, self.coin = sample, coin
        self._trace: Optional[List[_Step]] = None                 # tests set a list: every loss then appends its _Step

    # ---- targets ------------------------------------------------------------------------------------
    def prepare_targets(self, targets) -> List[List[Dict[str, Any]]]:
        """targets_list[f][b] = {labels, masks, inst_id, valid} of image b F + f.  Boxes are not read: the matcher does not use them."""
        F = self.sampling_frame_num
        if F < 1 or len(targets) % F:
            raise ValueError(f"CTCLPlugin: {len(targets)} images are not a multiple of sampling_frame_num = {F}")
        new = []
        for t in targets:
            if isinstance(t, dict):
                labels, masks, ids = t["labels"], t["masks"], t["ids"] if "ids" in t else t["inst_id"]
            else:
                labels, masks, ids = t.gt_classes, t.gt_masks, t.gt_ids
            masks = getattr(masks, "tensor", masks)               # detectron2's BitMasks
            new.append({"labels": labels, "masks": masks, "inst_id": ids})
        on_device = [t["inst_id"] for t in new if t["inst_id"].device.type != "cpu"]
        if on_device:                                             # one small copy for all images
            counts = [int(t["inst_id"].shape[0]) for t in new]
            host = torch.cat([t["inst_id"].reshape(-1).to(on_device[0].device) for t in new]).cpu().split(counts)
        else:
            host = [t["inst_id"] for t in new]
        for t, ids in zip(new, host):
            t["valid"] = ids != -1
        bz = len(new) // F
        return [[new[b * F + f] for b in range(bz)] for f in range(F)]

    # ---- the loss on given indices ------------------------------------------------------------------
    def _refuse(self, embeds: torch.Tensor, targets_list) -> None:
        F = self.sampling_frame_num
        if embeds.device.type != "cuda":
            raise RuntimeError("CTCLPlugin runs on the MI355X: CPU tensors are refused, move outputs and targets with .to('cuda') (there is no CPU fallback)")
        if embeds.dim() != 3:
            raise ValueError(f"CTCLPlugin: pred_embeds [B F, Q, C], got {tuple(embeds.shape)}")
        N, Q, C = embeds.shape
        if F < 1 or N % F or N != F * len(targets_list[0]) or len(targets_list) != F:
            raise ValueError(f"CTCLPlugin: {N} images are not sampling_frame_num = {F} frames of {len(targets_list[0])} videos")
        if C % 8 or not 8 <= C <= MAX_C:
            raise RuntimeError(f"CTCLPlugin: capacity limit: pred_embeds of {C} channels; the kernels take a multiple of 8 up to {MAX_C}")
        if F > MAX_F:
            raise RuntimeError(f"CTCLPlugin: capacity limit: sampling_frame_num = {F} exceeds {MAX_F}")
        if Q < self.num_negatives + 1:
            raise ValueError(f"CTCLPlugin: {Q} queries for num_negatives + 1 = {self.num_negatives + 1}")
        for b in range(len(targets_list[0])):
            counts = [int(targets_list[f][b]["valid"].shape[0]) for f in range(F)]
            if len(set(counts)) != 1:
                raise ValueError(f"CTCLPlugin: video {b}: its frames have differing instance counts {counts}")
            if counts[0] > Q:
                raise ValueError(f"CTCLPlugin: video {b}: {counts[0]} instances for {Q} queries")

    def plan(self, targets_list, indices_list, Q: int) -> Plan:
        F, B = self.sampling_frame_num, len(targets_list[0])
        valid = [[[bool(v) for v in targets_list[f][b]["valid"].tolist()] for f in range(F)] for b in range(B)]
        gt2query = []
        for b in range(B):
            per = []
            for f in range(F):
                src, tgt = indices_list[f][b]
                src, tgt = torch.as_tensor(src).reshape(-1), torch.as_tensor(tgt).reshape(-1)
                if src.numel() != len(valid[b][0]) or tgt.numel() != src.numel():
                    raise ValueError(f"CTCLPlugin: video {b}, frame {f}: {src.numel()} matched pairs for {len(valid[b][0])} instances")
                per.append(src[torch.sort(tgt)[1]].tolist())
            gt2query.append(per)
        return Plan(gt2query, valid, F, Q, self.num_negatives, self.momentum_embed, self.sample, self.coin)

    def get_reid_loss(self, targets_list, outputs_list, indices_list) -> Dict[str, torch.Tensor]:
        """The reference's signature: outputs_list[f]["pred_embeds"] [B, Q, C] per frame position."""
        embeds = torch.stack([o["pred_embeds"] for o in outputs_list], dim=1).flatten(0, 1)
        return self._reid(embeds, targets_list, indices_list)

    def _reid(self, embeds, targets_list, indices_list) -> Dict[str, torch.Tensor]:
        self._refuse(embeds, targets_list)
        plan = self.plan(targets_list, indices_list, int(embeds.shape[1]))
        if plan.I == 0:
            return {"loss_reid": embeds.sum() * 0, "loss_aux_reid": embeds.sum() * 0}
        step = _Step(plan, embeds)
        if self._trace is not None:
            self._trace.append(step)
        out = _ReidFunction.apply(step, embeds)
        return {"loss_reid": out[0], "loss_aux_reid": out[1]}

    # ---- the matching -------------------------------------------------------------------------------
    def _match(self, det_outputs, targets_list, matcher):
        F, B = self.sampling_frame_num, len(targets_list[0])
        layer = {k: v for k, v in det_outputs.items() if k not in ("aux_outputs", "interm_outputs")}
        if not isinstance(matcher, crit.HungarianMatcher):
            out = []
            for f in range(F):
                sel = torch.arange(f, B * F, F, device=det_outputs["pred_logits"].device)
                out.append(matcher({k: v[sel] for k, v in layer.items()}, targets_list[f]))
            return out
        dev = det_outputs["pred_logits"].device
        if B > crit.MAX_IMAGES:
            raise RuntimeError(f"CTCLPlugin: capacity limit: {B} videos exceed the matcher's {crit.MAX_IMAGES} images per call")
        draws = [[matcher.draw_points(1, dev) for _ in range(B)] for _ in range(F)]      # the reference's (position, image) order
        per = max(1, crit.MAX_IMAGES // B)                        # whole frame positions per call
        out: List[Any] = [None] * F
        for f0 in range(0, F, per):
            fs = list(range(f0, min(f0 + per, F)))
            images = [b * F + f for b in range(B) for f in fs]    # image order
            whole = len(images) == B * F
            sub = layer if whole else {k: layer[k][torch.as_tensor(images, device=dev)] for k in ("pred_logits", "pred_masks")}
            targets = [targets_list[n % F][n // F] for n in images]
            coords = torch.cat([draws[n % F][n // F] for n in images])[None]
            idx = matcher.match_layers([sub], targets, coords=coords)[0]
            for k, n in enumerate(images):
                if out[n % F] is None:
                    out[n % F] = [None] * B
                out[n % F][n // F] = idx[k]
        return out

    def train_loss(self, det_outputs, gt_instances, matcher) -> Dict[str, torch.Tensor]:
        embeds = det_outputs["pred_embeds"]
        targets_list = self.prepare_targets(gt_instances)
        self._refuse(embeds, targets_list)
        indices_list = self._match(det_outputs, targets_list, matcher)
        losses = self._reid(embeds, targets_list, indices_list)
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}


def ctvis_train_losses(det_outputs, targets, gt_instances, criterion, cl_plugin) -> Dict[str, torch.Tensor]:
    """``CTVISModel.train_model``'s losses: the criterion's with its ``weight_dict`` applied (other keys dropped), then the plugin's."""
    losses = criterion(det_outputs, targets)
    for k in list(losses.keys()):
        if k in criterion.weight_dict:
            losses[k] = losses[k] * criterion.weight_dict[k]
        else:
            losses.pop(k)
    losses.update(cl_plugin.train_loss(det_outputs, gt_instances, criterion.matcher))
    return losses
