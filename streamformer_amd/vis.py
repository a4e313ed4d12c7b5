"""Video instance segmentation end to end: the CTVIS tracker and mask post-processing over the native mask decoder's per-frame outputs.

Mirrors of the reference's ``SimpleTracker`` + ``MemoryBank`` (``downstream/OVIS/ctvis/modeling/tracker/``), of ``mask_nms``
(``ctvis/utils/utils.py``) and of the inference branch of ``CTVISModel`` (``ctvis/ctvis_model.py``: ``inference_model`` and
``inference_video``), restated over four kernels of ``libstreamformer_hip.so`` (``csrc/sf_vis.hip``):

    det = mask_decoder(multi_scale_features, mask_features)              # pred_logits, pred_masks, pred_embeds, pred_queries per frame
    tracker = SimpleTracker(num_classes=40)
    out = tracker.inference(det, dense_masks=False)                      # pred_logits [1, K, C + 1], det_masks [F Q, h, w], mask_index [K, F]
    video = postprocess_video_masks(out["pred_logits"], (out["det_masks"], out["mask_index"]), image_tensor_size, image_size,
                                    height, width, num_classes=40, num_topk=10)

Where things run.  What is frame-local and state-free runs on the GPU for all frames of a clip in three launches before the loop starts:
the softmax scores and labels (``sf_op_vis_scores``), the bit-packed masks ``x > 0`` with their areas (``sf_op_vis_pack_masks``) and the
pairwise intersections inside each frame (``sf_op_vis_mask_iou``).  ONE device-to-host copy (``_device_to_host``, the only one inside
``SimpleTracker.inference`` / ``step``) then brings scores, labels, logits, intersections, areas, ``pred_embeds`` and ``pred_queries`` to the host, where the data-dependent
loop (selection, the NMS scan, similarity, matching, memory bank, the dead-tracklet and noise-sequence rules) runs in fp32 torch CPU ops
without a further synchronisation.  Masks never leave the device: the loop carries row indices into the detections' ``pred_masks``, and
``sf_op_vis_postprocess`` gathers and resamples them.  There is no CPU fallback for the kernels; the host loop alone is reachable
without a GPU through ``step_host`` (tests feed it precomputed scores and intersections).  ``postprocess_video_masks`` ends, as the
reference's ``inference_video`` does, by bringing its results to the caller: ``tolist()`` of the scores and labels and the masks'
``.to(to_store)`` are device-to-host copies of their own, after the kernel.  The kernels allocate nothing and take one workspace (the
post-processing kernel's block partials); the Python layer makes each call's output tensors through torch's caching allocator.

Memory of an online caller: between ``reset()`` and ``finish()`` the tracker keeps every stepped frame's detection masks
(``det_masks``, Q h w fp32 values per frame on the device: about 10 MB per frame at Q = 100, 120 x 214) because ``finish()``'s index
table names rows of them, and one ``trace`` entry per frame on the host.  Both grow with the number of frames and are dropped by
``reset()``; the reference, which keeps only the tracked instances' masks, grows with instances x frames instead.

Where this differs from the reference, on purpose: ``mask_nms`` thresholds ``sigmoid(x) > 0.5``, which is ``x > 0`` except for logits
below one rounding of 0.5 (|x| < 2.4e-7 in fp32), and the packed rule is ``x > 0``; a frame that finds the memory bank empty although
tracklets existed (all dead) starts new tracklets where the reference fails in ``torch.stack([])``; a tracker without any instance
returns ``pred_masks=[]`` next to ``pred_logits=[]``; ``num_topk`` above the number of scores takes them all.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn
import torch.nn.functional as F

from . import _native as nat

__all__ = ["SimpleTracker", "postprocess_video_masks", "VideoInstanceSegmenter"]

MATCH_METRICS = ("bisoftmax", "cosine")
MATCH_TYPES = ("greedy", "hungarian")
EMBED_TYPES = ("last", "temporally_weighted_softmax", "momentum", "similarity_guided")
TEMPORAL_SCORE_TYPES = ("mean", "max")
MOMENTUM = 0.75
HOST_KEYS = ("max_scores", "labels", "pred_logits", "inter", "area", "pred_embeds", "pred_queries")


def _device_to_host(buffer: torch.Tensor) -> torch.Tensor:
    """The tracker's single device-to-host copy per clip (``inference``) or per frame (``step``); synchronises the stream."""
    return buffer.cpu()


def _require_cuda(what: str, *tensors: torch.Tensor) -> torch.device:
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(f"{what} runs on the MI355X: move its inputs with .to('cuda') (there is no CPU fallback)")
    return tensors[0].device


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def vis_scores(pred_logits: torch.Tensor, full: bool = False):
    """``pred_logits`` [..., C + 1] on the GPU -> (max_scores [...], labels [...] int32, scores [..., C] or None)."""
    dev = _require_cuda("sf_op_vis_scores", pred_logits)
    x = _f32(pred_logits)
    lead, c1 = x.shape[:-1], x.shape[-1]
    rows = int(math.prod(lead))
    mx = torch.empty(lead, dtype=torch.float32, device=dev)
    lab = torch.empty(lead, dtype=torch.int32, device=dev)
    sc = torch.empty(lead + (c1 - 1,), dtype=torch.float32, device=dev) if full else None
    nat.launch(dev, nat.lib.sf_op_vis_scores, x.data_ptr(), rows, c1, mx.data_ptr(), lab.data_ptr(), nat.ptr(sc))
    return mx, lab, sc


def resample_masks(det_masks: torch.Tensor, index: torch.Tensor, padded: Tuple[int, int], crop: Tuple[int, int], out: Tuple[int, int], *,
                   masks: bool = True, logits: bool = False, sums: bool = True, workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``sf_op_vis_postprocess``: ``det_masks`` [R, h, w] fp32 and ``index`` [K, F] int32 (a row, or -1) on the GPU -> any of ``masks``
    bool [K, F, H, W], ``logits`` fp32 [K, F, H, W], ``numerator`` fp32 [K] with ``denominator`` int64 [K]."""
    dev = _require_cuda("sf_op_vis_postprocess", det_masks, index)
    if det_masks.dim() != 3 or index.dim() != 2:
        raise ValueError(f"det_masks must be (R, h, w) and index (K, F), got {tuple(det_masks.shape)} and {tuple(index.shape)}")
    src, idx = _f32(det_masks), index.to(torch.int32).contiguous()
    (R, h, w), (K, Fr), (H, W) = src.shape, idx.shape, out
    res: Dict[str, torch.Tensor] = {}
    if masks:
        res["masks"] = torch.empty(K, Fr, H, W, dtype=torch.bool, device=dev)
    if logits:
        res["logits"] = torch.empty(K, Fr, H, W, dtype=torch.float32, device=dev)
    if sums:
        res["numerator"] = torch.empty(K, dtype=torch.float32, device=dev)
        res["denominator"] = torch.empty(K, dtype=torch.int64, device=dev)
        need = nat.lib.sf_op_vis_postprocess_workspace_bytes(K, Fr, H, W)
        if workspace is None or workspace.numel() < need or workspace.device != dev:
            workspace = nat.scratch(need, dev)
    nat.launch(dev, nat.lib.sf_op_vis_postprocess, src.data_ptr(), R, h, w, idx.data_ptr(), K, Fr, padded[0], padded[1], crop[0], crop[1], H, W,
               nat.ptr(res.get("masks")), nat.ptr(res.get("logits")), nat.ptr(res.get("numerator")), nat.ptr(res.get("denominator")),
               workspace=workspace if sums else None)
    return res


class _Tracklet:
    """One tracklet of the memory bank: the cached scores and embeddings, the momentum and the similarity-guided embedding."""

    def __init__(self):
        self.scores: List[torch.Tensor] = []
        self.embeds: List[torch.Tensor] = []
        self.last_frame = -1
        self.exist_frames = 0
        self.momentum_embed = self.guided_embed = None

    def update(self, score: torch.Tensor, embed: torch.Tensor, frame_id: int, maximum_cache: int) -> None:
        self.scores.append(score)
        self.embeds.append(embed)
        self.last_frame = frame_id
        if self.exist_frames == 0:
            self.momentum_embed = self.guided_embed = embed
        else:
            self.momentum_embed = (1 - MOMENTUM) * self.momentum_embed + MOMENTUM * embed
            earlier = F.normalize(torch.stack(self.embeds[:-1], dim=0), dim=-1)
            similarity = torch.sum(earlier @ F.normalize(embed, dim=-1)) / (len(self.embeds) - 1)
            beta = torch.clamp(similarity, min=0)
            self.guided_embed = (1 - beta) * self.guided_embed + beta * embed
        self.exist_frames += 1
        if len(self.scores) > maximum_cache:
            self.scores.pop(0)
            self.embeds.pop(0)

    def embed(self, embed_type: str) -> torch.Tensor:
        if embed_type == "last":
            return self.embeds[-1]
        if embed_type == "momentum":
            return self.momentum_embed
        if embed_type == "similarity_guided":
            return self.guided_embed
        scores = torch.stack(self.scores)                    # temporally_weighted_softmax
        n = scores.shape[0]
        step = 1 / n                                         # torch.range(0., 1, 1 / n)[1:]: fp32 roundings of i * step, formed in fp64
        count = int(math.floor(1.0 / step + 1)) - 1
        temporal = torch.tensor([(i + 1) * step for i in range(count)], dtype=torch.float64).to(torch.float32).to(scores)
        weights = scores + temporal
        return (torch.stack(self.embeds) * weights.unsqueeze(1)).sum(0) / weights.sum()


class SimpleTracker(nn.Module):
    """The reference's ``SimpleTracker`` (IDOL-style online association) with its explicit-keyword constructor; defaults are those of
    ``ctvis/config.py``.  ``inference`` is ``reset`` + ``step`` x F + ``finish`` with the frame-local front batched over the clip."""

    def __init__(self, *, num_classes: int, match_metric: str = "bisoftmax", frame_weight: bool = True, match_score_thr: float = 0.2,
                 temporal_score_type: str = "mean", match_type: str = "greedy", inference_select_thr: float = 0.01, init_score_thr: float = 0.01,
                 mask_nms_thr: float = 0.6, num_dead_frames: int = 20, embed_type: str = "similarity_guided", maximum_cache: int = 10,
                 noise_frame_num: int = 8, noise_frame_ratio: float = 0.4, suppress_frame_num: int = 3, none_frame_num: int = 2):
        super().__init__()
        if temporal_score_type == "hybrid":
            raise NotImplementedError("temporal_score_type='hybrid' is not implemented (the reference raises NotImplementedError for it too)")
        for name, value, allowed in (("match_metric", match_metric, MATCH_METRICS), ("match_type", match_type, MATCH_TYPES),
                                     ("embed_type", embed_type, EMBED_TYPES), ("temporal_score_type", temporal_score_type, TEMPORAL_SCORE_TYPES)):
            if value not in allowed:
                raise NotImplementedError(f"{name}={value!r} is not implemented: one of {allowed}")
        if match_type == "hungarian":
            try:
                from scipy.optimize import linear_sum_assignment      # noqa: F401
            except ImportError as e:
                raise ImportError("match_type='hungarian' needs scipy (scipy.optimize.linear_sum_assignment)") from e
        self.num_classes, self.match_metric, self.frame_weight = int(num_classes), match_metric, bool(frame_weight)
        self.match_score_thr, self.temporal_score_type, self.match_type = match_score_thr, temporal_score_type, match_type
        self.inference_select_thr, self.init_score_thr, self.mask_nms_thr = inference_select_thr, init_score_thr, mask_nms_thr
        self.num_dead_frames, self.embed_type, self.maximum_cache = num_dead_frames, embed_type, maximum_cache
        self.noise_frame_num, self.noise_frame_ratio = noise_frame_num, noise_frame_ratio
        self.suppress_frame_num, self.none_frame_num = suppress_frame_num, none_frame_num
        self.reset()

    # ------------------------------------------------------------------------------------ state
    def reset(self) -> None:
        self.num_tracklets = 0
        self.tracklets: Dict[int, _Tracklet] = {}            # the memory bank, in insertion order
        self.video: Dict[int, Dict[str, list]] = {}          # instance id -> per frame a row of the detections' masks (or None) and its logits
        self.frame_id = 0
        self.det_masks: List[torch.Tensor] = []              # the detections' pred_masks, on the device, one entry per step
        self.trace: List[Dict[str, Any]] = []                # per frame what was kept and assigned (tests, debugging)

    @property
    def empty(self) -> bool:
        return self.num_tracklets == 0

    # ------------------------------------------------------------------------------------ the frame-local front (GPU)
    def _front(self, det: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Scores, labels, packed masks, areas and intersections of every frame in three launches, then the one copy to the host."""
        logits, masks = det["pred_logits"], det["pred_masks"]
        dev = _require_cuda("the tracker's front", logits, masks, det["pred_embeds"], det["pred_queries"])
        if logits.dim() != 3 or masks.dim() != 4 or masks.shape[:2] != logits.shape[:2]:
            raise ValueError(f"pred_logits must be (F, Q, C + 1) and pred_masks (F, Q, h, w), got {tuple(logits.shape)} and {tuple(masks.shape)}")
        if logits.shape[-1] != self.num_classes + 1:
            raise ValueError(f"pred_logits has {logits.shape[-1]} columns, the tracker was made for {self.num_classes} classes + 1")
        Fr, Q = logits.shape[:2]
        pixels = masks.shape[2] * masks.shape[3]
        lg, mk = _f32(logits), _f32(masks)
        mx, lab, _ = vis_scores(lg)
        bits = torch.empty(Fr, Q, (pixels + 31) // 32, dtype=torch.int32, device=dev)
        area = torch.empty(Fr, Q, dtype=torch.int32, device=dev)
        inter = torch.empty(Fr, Q, Q, dtype=torch.int32, device=dev)
        nat.launch(dev, nat.lib.sf_op_vis_pack_masks, mk.data_ptr(), Fr * Q, pixels, bits.data_ptr(), area.data_ptr())
        nat.launch(dev, nat.lib.sf_op_vis_mask_iou, bits.data_ptr(), Fr, Q, pixels, inter.data_ptr())
        parts = dict(zip(HOST_KEYS, (mx, lab, lg, inter, area, _f32(det["pred_embeds"]), _f32(det["pred_queries"]))))
        flat = torch.cat([(t if t.dtype == torch.float32 else t.view(torch.float32)).reshape(-1) for t in parts.values()])
        host_flat = _device_to_host(flat)
        host, off = {}, 0
        for k, t in parts.items():
            piece = host_flat[off:off + t.numel()]
            host[k] = (piece if t.dtype == torch.float32 else piece.view(torch.int32)).view(t.shape)
            off += t.numel()
        host["det_masks"] = mk.view(Fr * Q, masks.shape[2], masks.shape[3])
        return host

    # ------------------------------------------------------------------------------------ the sequential loop (host)
    def step(self, frame_outputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """One frame (tensors [Q, ...] or [1, Q, ...] on the GPU) for a caller that gets frames one at a time; returns the frame's ids."""
        det = {k: (frame_outputs[k] if frame_outputs[k].dim() == (4 if k == "pred_masks" else 3) else frame_outputs[k][None])
               for k in ("pred_logits", "pred_masks", "pred_embeds", "pred_queries")}
        if det["pred_logits"].shape[0] != 1:
            raise ValueError("step() takes one frame; inference() takes a clip")
        host = self._front(det)
        self.det_masks.append(host["det_masks"])
        return self.step_host(*(host[k][0] for k in ("max_scores", "pred_logits", "inter", "area", "pred_embeds", "pred_queries")))

    def step_host(self, max_scores: torch.Tensor, pred_logits: torch.Tensor, inter: torch.Tensor, area: torch.Tensor, pred_embeds: torch.Tensor,
                  pred_queries: torch.Tensor) -> torch.Tensor:
        """The loop's body over host tensors of one frame: ``max_scores`` [Q], ``pred_logits`` [Q, C + 1], ``inter`` [Q, Q] and ``area`` [Q]
        (integers), ``pred_embeds`` and ``pred_queries`` [Q, E].  Detections are named by their row ``frame * Q + query``."""
        del pred_queries                                     # collected by the reference, never used in what it returns
        frame_id, Q = self.frame_id, max_scores.shape[0]
        order = torch.sort(max_scores, dim=0, descending=True)[1]
        scores = max_scores[order]
        valid = scores > self.inference_select_thr
        if valid.sum() == 0:
            valid[0] = True
        order, scores = order[valid], scores[valid]
        selected = order.tolist()
        # mask NMS over the selection, in score order, from the intersections and areas
        i_sel = inter[order][:, order].to(scores.dtype)
        a_sel = area[order].to(scores.dtype)
        iou = (i_sel + 1e-6) / (a_sel[:, None] + a_sel[None, :] - i_sel + 1e-6)
        over = (iou > self.mask_nms_thr).tolist()
        keep = [True] * len(selected)
        for i in range(len(selected) - 1):
            if keep[i]:
                for j in range(i + 1, len(selected)):
                    if keep[j] and over[i][j]:
                        keep[j] = False
        keep_t = torch.tensor(keep)
        order, scores = order[keep_t], scores[keep_t]
        embeds, logits = pred_embeds[order], pred_logits[order]
        seen: Dict[str, Any] = {"bank_ids": list(self.tracklets) if not self.empty else [], "bank_embeds": None, "match": None}
        ids = self._assign(scores, embeds, frame_id, seen)
        tracked = ids > -1
        ids_l = ids[tracked].tolist()
        for k, inst in zip(torch.nonzero(tracked).flatten().tolist(), ids_l):
            if inst not in self.tracklets:
                self.tracklets[inst] = _Tracklet()
            self.tracklets[inst].update(scores[k], embeds[k], frame_id, self.maximum_cache)
            entry = self.video.setdefault(inst, {"rows": [None] * frame_id, "logits": [None] * frame_id})
            entry["rows"].append(frame_id * Q + int(order[k]))
            entry["logits"].append(logits[k])
        for dead in [i for i, t in self.tracklets.items() if frame_id - t.last_frame > self.num_dead_frames]:
            del self.tracklets[dead]
        for entry in self.video.values():
            if len(entry["rows"]) < frame_id + 1:
                entry["rows"].append(None)
                entry["logits"].append(None)
        if frame_id > self.noise_frame_num:                  # short sequences that have stopped are noise
            for inst in list(self.video):
                rows = self.video[inst]["rows"]
                present = sum(r is not None for r in rows)
                trailing = next((n for n, r in enumerate(reversed(rows)) if r is not None), len(rows))
                if trailing >= self.none_frame_num and present < self.suppress_frame_num:
                    del self.video[inst]                     # the memory bank keeps its tracklet, as in the reference
        self.trace.append({**seen, "selected": selected, "kept": order.tolist(), "ids": ids_l, "tracked": [int(q) for q in order[tracked].tolist()]})
        self.frame_id += 1
        return ids[tracked]

    def _assign(self, scores: torch.Tensor, embeds: torch.Tensor, frame_id: int, seen: Dict[str, Any]) -> torch.Tensor:
        ids = torch.full((scores.shape[0],), -1, dtype=torch.long)
        if not self.empty and self.tracklets:
            exist_ids = list(self.tracklets)
            exist_embeds = torch.stack([t.embed(self.embed_type) for t in self.tracklets.values()], dim=0)
            exist_frames = torch.tensor([t.exist_frames for t in self.tracklets.values()], dtype=torch.long)
            if self.match_metric == "bisoftmax":
                similarity = torch.mm(embeds, exist_embeds.t())
                match = (similarity.softmax(dim=1) + similarity.softmax(dim=0)) / 2
            else:
                match = torch.mm(F.normalize(embeds, p=2, dim=1), F.normalize(exist_embeds, p=2, dim=1).t())
            thr = self.match_score_thr
            seen.update(bank_embeds=exist_embeds, match=match.clone())     # what the frame was matched against, before the greedy loop edits it
            if self.match_type == "greedy":
                for i in range(scores.shape[0]):
                    row = match[i]
                    above = row > thr
                    if self.frame_weight and int(above.sum()) > 1:
                        weight = exist_frames[above].to(row)
                        row = torch.where(above, row * exist_frames.to(row), row * weight.mean())
                    best, col = torch.max(row, dim=0)
                    if best > thr:
                        ids[i] = exist_ids[int(col)]
                        taken = match[i, col].clone()
                        match[:, col] = 0
                        match[i, col] = taken
            else:
                from scipy.optimize import linear_sum_assignment
                rows, cols = linear_sum_assignment((-match).numpy())
                for r, c in zip(rows, cols):
                    if not match[r, c] < thr:
                        ids[r] = exist_ids[c]
        new = (ids == -1) & (scores > self.init_score_thr)
        count = int(new.sum())
        ids[new] = torch.arange(self.num_tracklets, self.num_tracklets + count, dtype=torch.long)
        self.num_tracklets += count
        return ids

    # ------------------------------------------------------------------------------------ results
    def finish(self, dense_masks: bool = False) -> Dict[str, Any]:
        """``pred_logits`` [1, K, C + 1] (or ``[]``), ``mask_index`` int32 [K, F]: per instance and frame a row of ``det_masks``
        [F Q, h, w], or -1 where the instance is absent.  ``dense_masks`` adds the reference's ``pred_masks`` [1, K, F, h, w]."""
        Fr = self.frame_id
        logits, table = [], []
        for entry in self.video.values():
            seen = torch.stack([l for l in entry["logits"] if l is not None])
            logits.append(seen.mean(0) if self.temporal_score_type == "mean" else seen.max(0)[0])
            table.append([-1 if r is None else r for r in entry["rows"]])
        if not logits:
            return {"pred_logits": [], "pred_masks": [], "mask_index": torch.empty(0, Fr, dtype=torch.int32), "det_masks": None}
        out: Dict[str, Any] = {"pred_logits": torch.stack(logits, dim=0)[None], "mask_index": torch.tensor(table, dtype=torch.int32), "det_masks": None}
        if self.det_masks:
            det = self.det_masks[0] if len(self.det_masks) == 1 else torch.cat(self.det_masks, dim=0)
            self.det_masks = [det]
            dev = det.device
            out.update(det_masks=det, pred_logits=out["pred_logits"].to(dev), mask_index=out["mask_index"].to(dev))
            if dense_masks:
                hw = tuple(det.shape[1:])
                out["pred_masks"] = resample_masks(det, out["mask_index"], hw, hw, hw, masks=False, logits=True, sums=False)["logits"][None]
        elif dense_masks:
            raise RuntimeError("dense masks are gathered on the MI355X from the detections' pred_masks: none were given (step_host carries rows only)")
        return out

    def inference(self, det_outputs: Dict[str, torch.Tensor], hybrid_embed: Any = None, dense_masks: bool = True) -> Dict[str, Any]:
        """The reference's ``inference``: ``det_outputs`` with ``pred_logits`` [F, Q, C + 1], ``pred_masks`` [F, Q, h, w], ``pred_embeds``
        and ``pred_queries`` [F, Q, E] on the GPU.  ``hybrid_embed`` is accepted and unused, as in the reference."""
        del hybrid_embed
        self.reset()
        host = self._front(det_outputs)
        self.det_masks.append(host["det_masks"])
        for f in range(host["max_scores"].shape[0]):
            self.step_host(*(host[k][f] for k in ("max_scores", "pred_logits", "inter", "area", "pred_embeds", "pred_queries")))
        return self.finish(dense_masks=dense_masks)

    def forward(self, *args, **kwargs):
        return self.inference(*args, **kwargs)


def _empty_video(image_size) -> Dict[str, Any]:
    return {"image_size": image_size, "pred_scores": [], "pred_labels": [], "pred_masks": []}


@torch.no_grad()
def postprocess_video_masks(pred_logits: Any, pred_masks: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], image_tensor_size: Sequence[int],
                            image_size: Sequence[int], height: int, width: int, num_classes: int, num_topk: int, to_store: Any = "cpu",
                            test_interpolate_chunk_size: Optional[int] = None, test_instance_chunk_size: Optional[int] = None) -> Dict[str, Any]:
    """The reference's ``inference_video``.  ``pred_logits`` [1, K, C + 1]; ``pred_masks`` the tracker's dense [1, K, F, h, w] or its
    ``(det_masks [R, h, w], mask_index [K, F])``; ``image_tensor_size`` the padded batch's shape (its last two entries are used),
    ``image_size`` the first frame's size before padding, ``height`` x ``width`` the video's own resolution.  Returns ``image_size``,
    ``pred_scores`` and ``pred_labels`` (Python lists) and ``pred_masks``, one bool tensor [F, H, W] per instance on ``to_store``.

    The two chunk sizes are accepted and ignored: the reference chunks to bound the [K, F, H_pad, W_pad] intermediate of its first
    ``F.interpolate``; the native kernel composes both resamples per output pixel and forms no intermediate, so there is nothing to
    chunk."""
    del test_interpolate_chunk_size, test_instance_chunk_size
    height, width = int(height), int(width)
    if len(pred_logits) == 0 or len(pred_logits[0]) == 0:
        return _empty_video((height, width))
    cls = pred_logits[0]
    if isinstance(pred_masks, (tuple, list)):
        det, index = pred_masks
    else:
        dense = pred_masks[0]
        det = dense.reshape((-1,) + tuple(dense.shape[2:]))
        index = torch.arange(det.shape[0], dtype=torch.int32, device=det.device).view(dense.shape[:2])
    dev = _require_cuda("postprocess_video_masks", cls, det, index)
    if cls.shape[-1] != num_classes + 1:
        raise ValueError(f"pred_logits has {cls.shape[-1]} columns, expected num_classes + 1 = {num_classes + 1}")
    scores = vis_scores(cls, full=True)[2]
    top_scores, top = scores.flatten(0, 1).topk(min(int(num_topk), scores.numel()), sorted=True)
    labels = top % num_classes
    picked = index.to(torch.int32)[top // num_classes]
    res = resample_masks(det, picked, (int(image_tensor_size[-2]), int(image_tensor_size[-1])), (int(image_size[0]), int(image_size[1])), (height, width))
    top_scores = top_scores * (res["numerator"] / (res["denominator"].to(torch.float32) + 1e-6))
    stored = res["masks"].to(to_store)
    return {"image_size": (height, width), "pred_scores": top_scores.tolist(), "pred_labels": labels.tolist(), "pred_masks": [m for m in stored]}


class VideoInstanceSegmenter(nn.Module):
    """The inference branch of ``CTVISModel.forward`` over the three native modules and the tracker: normalise and pad the frames to
    ``size_divisibility``, run windows of ``num_clip_frames`` frames (the last one ragged) through backbone, pixel decoder and mask
    decoder, concatenate, track, post-process.  Holds the modules and adds no parameters."""

    def __init__(self, backbone: nn.Module, pixel_decoder: nn.Module, mask_decoder: nn.Module, tracker: SimpleTracker, *, num_topk: int,
                 num_clip_frames: int = 16, size_divisibility: int = 32, pixel_mean: Sequence[float] = (123.675, 116.28, 103.53),
                 pixel_std: Sequence[float] = (58.395, 57.12, 57.375), to_cpu_frames: int = 40, test_interpolate_chunk_size: int = 5,
                 test_instance_chunk_size: int = 5):
        super().__init__()
        self.backbone, self.pixel_decoder, self.mask_decoder, self.tracker = backbone, pixel_decoder, mask_decoder, tracker
        self.num_topk, self.num_clip_frames, self.size_divisibility = int(num_topk), int(num_clip_frames), int(size_divisibility)
        self.to_cpu_frames = int(to_cpu_frames)
        self.test_interpolate_chunk_size, self.test_instance_chunk_size = test_interpolate_chunk_size, test_instance_chunk_size
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), persistent=False)

    @property
    def device(self) -> torch.device:
        return self.pixel_mean.device

    def pre_process(self, batched_inputs: List[Dict[str, Any]]) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
        """The normalised frames padded (bottom and right, zeros) to one size that ``size_divisibility`` divides, and each frame's own size."""
        images = [(frame.to(self.device) - self.pixel_mean) / self.pixel_std for video in batched_inputs for frame in video["image"]]
        sizes = [(int(x.shape[-2]), int(x.shape[-1])) for x in images]
        d = max(self.size_divisibility, 1)
        Hp = (max(s[0] for s in sizes) + d - 1) // d * d
        Wp = (max(s[1] for s in sizes) + d - 1) // d * d
        batch = images[0].new_zeros(len(images), images[0].shape[0], Hp, Wp)
        for i, x in enumerate(images):
            batch[i, :, :x.shape[-2], :x.shape[-1]] = x
        return batch, sizes

    @torch.no_grad()
    def detect(self, frames: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``frames`` [N, 3, Hp, Wp], padded: the decoder's per-frame outputs over windows of ``num_clip_frames`` frames, concatenated."""
        keys = ("pred_logits", "pred_masks", "pred_embeds", "pred_queries")
        parts: Dict[str, List[torch.Tensor]] = {k: [] for k in keys}
        for start in range(0, frames.shape[0], self.num_clip_frames):
            clip = frames[start:start + self.num_clip_frames]
            features = self.backbone(pixel_values=clip.reshape(1, -1, *clip.shape[1:]), output_attentions=False, output_hidden_states=True,
                                     return_dict=True)
            mask_features, _, multi_scale = self.pixel_decoder.forward_features(features)
            out = self.mask_decoder(multi_scale, mask_features)
            for k in keys:
                parts[k].append(out[k])
        return {k: v[0] if len(v) == 1 else torch.cat(v, dim=0) for k, v in parts.items()}

    @torch.no_grad()
    def forward(self, batched_inputs: List[Dict[str, Any]]) -> Dict[str, Any]:
        """``batched_inputs``: one video, ``{"image": [frames (3, H, W)], "height": .., "width": ..}`` (the last two default to the first
        frame's size).  Returns the reference's ``video_output``."""
        if self.training:
            raise NotImplementedError("VideoInstanceSegmenter is inference only: call .eval() (training, the losses and ct_cl_plugin are not part of it)")
        frames, sizes = self.pre_process(batched_inputs)
        to_store = self.device if len(sizes) <= self.to_cpu_frames else "cpu"
        tracked = self.tracker.inference(self.detect(frames), hybrid_embed=getattr(self.mask_decoder, "class_embed", None), dense_masks=False)
        if len(tracked["pred_logits"]) == 0:
            return _empty_video((sizes[0], sizes[min(1, len(sizes) - 1)]))      # the reference's empty dict: its first two frames' sizes
        first = batched_inputs[0]
        return postprocess_video_masks(tracked["pred_logits"], (tracked["det_masks"], tracked["mask_index"]), tuple(frames.shape), sizes[0],
                                       first.get("height", sizes[0][0]), first.get("width", sizes[0][1]), self.tracker.num_classes, self.num_topk,
                                       to_store, self.test_interpolate_chunk_size, self.test_instance_chunk_size)
