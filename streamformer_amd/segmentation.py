"""Image segmentation end to end: semantic, panoptic and instance outputs over the native mask decoder's per-image outputs.

Mirrors of the three inference functions and of the eval branch of the reference's ``TimesformerMaskFormer``
(``downstream/OVIS/mask2former/timesformer_maskformer_model.py``; the same three functions as ``maskformer_model.py``), restated over the
kernels of ``csrc/sf_seg.hip`` and ``csrc/sf_vis.hip``:

    out = mask_decoder(multi_scale_features, mask_features)              # pred_logits [B, Q, C + 1], pred_masks [B, Q, h, w]
    geometry = dict(padded=(Hp, Wp), crop=image_size, out=(height, width))
    sem = semantic_inference(out["pred_logits"][0], out["pred_masks"][0], geometry)                       # [C, height, width]
    pan, info = panoptic_inference(out["pred_logits"][0], out["pred_masks"][0], geometry, num_classes=C, object_mask_threshold=0.8,
                                   overlap_threshold=0.8, thing_classes=range(80))
    inst = instance_inference(out["pred_logits"][0], out["pred_masks"][0], geometry, num_classes=C, test_topk_per_image=100)

``geometry`` is what the reference does to a mask between the decoder and the result: ``F.interpolate`` from ``h x w`` to the padded
batch's ``padded`` size, ``sem_seg_postprocess`` (keep the top left ``crop`` = the image's own size, ``F.interpolate`` to ``out``).  The
kernels compose both resamples per output pixel (``sf_op_vis_postprocess``'s arithmetic) and form neither intermediate.

Where things run.  Everything per pixel runs on the GPU: the semantic contraction (``sf_op_seg_semantic``, fp32 MFMA), the panoptic
argmax over the kept queries with its three integer counts per query (``sf_op_seg_panoptic_argmax``; which queries are kept is decided on
the device, nothing is copied before the launch), the relabelling (``sf_op_seg_panoptic_relabel``), and for instances the top-k masks
with their score sums (``sf_op_vis_postprocess`` with an index table [K, 1]).  ``panoptic_inference`` makes ONE device-to-host copy
(``_device_to_host``: scores, labels, counts) for the data-dependent segment rule, ``panoptic_segments_host``, which is plain Python over
3 Q integers and reachable without a GPU.  There is no CPU fallback for the kernels.

Where this differs from the reference, on purpose: a pixel belongs to its winner's segment where the resampled logit ``r >= 0``, the
reference's ``sigmoid(r) >= 0.5`` except for logits below one rounding of 0.5 (-6e-8 <= r < 0 in fp32), as ``vis.py`` documents for
``x > 0``; ``instance_inference`` returns its instances sorted by class score, descending, where the reference's ``topk(sorted=False)``
leaves the order unspecified; ``test_topk_per_image`` above the number of scores takes them all.
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _native as nat
from .vis import VideoInstanceSegmenter, _f32, _require_cuda, resample_masks, vis_scores

__all__ = ["semantic_inference", "panoptic_inference", "panoptic_segments_host", "instance_inference", "SegmentationInstances", "ImageSegmenter"]

Geometry = Dict[str, Sequence[int]]


def _device_to_host(buffer: torch.Tensor) -> torch.Tensor:
    """``panoptic_inference``'s single device-to-host copy; synchronises the stream."""
    return buffer.cpu()


def _sizes(geometry: Geometry) -> Tuple[Tuple[int, int], Tuple[int, int], Tuple[int, int]]:
    padded, crop, out = (tuple(int(v) for v in geometry[k]) for k in ("padded", "crop", "out"))
    return padded, crop, out


def _check(mask_cls: torch.Tensor, mask_pred: torch.Tensor) -> None:
    if mask_cls.dim() != 2 or mask_pred.dim() != 3 or mask_cls.shape[0] != mask_pred.shape[0] or mask_cls.shape[1] < 2:
        raise ValueError(f"mask_cls must be (Q, C + 1) and mask_pred (Q, h, w), got {tuple(mask_cls.shape)} and {tuple(mask_pred.shape)}")


@torch.no_grad()
def semantic_inference(mask_cls: torch.Tensor, mask_pred: torch.Tensor, geometry: Geometry, *, postprocess_before_inference: bool = True) -> torch.Tensor:
    """The reference's ``semantic_inference`` with the resampling around it: ``mask_cls`` [Q, C + 1], ``mask_pred`` [Q, h, w] on the GPU
    -> fp32 [C, H, W], ``sum_q softmax(mask_cls)[q, c] sigmoid(resampled mask_pred[q])``.

    ``postprocess_before_inference=True`` resamples the masks to the output size first (``sem_seg_postprocess`` before the function, the
    composed geometry).  ``False`` is the reference's other order: the map is made at the padded size and the MAP is cropped and
    resampled.  The sigmoid does not commute with the resample, so the two differ."""
    _check(mask_cls, mask_pred)
    dev = _require_cuda("sf_op_seg_semantic", mask_cls, mask_pred)
    padded, crop, out = _sizes(geometry)
    probs = vis_scores(mask_cls, full=True)[2]
    src = _f32(mask_pred)
    (Q, h, w), C = src.shape, probs.shape[1]
    first_crop, first_out = (crop, out) if postprocess_before_inference else (padded, padded)
    sem = torch.empty((C,) + first_out, dtype=torch.float32, device=dev)
    nat.launch(dev, nat.lib.sf_op_seg_semantic, src.data_ptr(), probs.data_ptr(), Q, C, h, w, padded[0], padded[1], first_crop[0], first_crop[1],
               first_out[0], first_out[1], sem.data_ptr())
    if postprocess_before_inference:
        return sem
    index = torch.arange(C, dtype=torch.int32, device=dev).view(C, 1)
    return resample_masks(sem, index, padded, crop, out, masks=False, logits=True, sums=False)["logits"][:, 0]


def panoptic_segments_host(scores: Sequence[float], labels: Sequence[int], counts: Sequence[Sequence[int]], *, num_classes: int,
                           object_mask_threshold: float, overlap_threshold: float, thing_classes: Iterable[int]) -> Tuple[List[Dict[str, Any]], List[int]]:
    """The loop of the reference's ``panoptic_inference`` over what the argmax kernel counted: ``scores`` [Q] and ``labels`` [Q] (the
    largest softmax score over all C + 1 columns and its index), ``counts`` [Q][3] = (``mask_area``: pixels won, ``original_area``: pixels
    with ``r >= 0``, pixels with both).  Returns ``segments_info`` (``id``, ``isthing``, ``category_id``) and per query its segment id, 0
    where it has none.  Queries are walked in query order, which is the reference's order of the kept queries; segment ids count up from
    1; a stuff class seen before merges into its first segment (``stuff_memory_list``)."""
    things = set(int(c) for c in thing_classes)
    thr = float(torch.tensor(object_mask_threshold, dtype=torch.float32))      # the kernel's comparison is fp32
    segments_info: List[Dict[str, Any]] = []
    segment_of_query = [0] * len(labels)
    stuff_memory_list: Dict[int, int] = {}
    current_segment_id = 0
    for q, (score, label) in enumerate(zip(scores, labels)):
        pred_class = int(label)
        if pred_class == num_classes or not float(score) > thr:
            continue
        mask_area, original_area, both = (int(v) for v in counts[q])
        if mask_area > 0 and original_area > 0 and both > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            isthing = pred_class in things
            if not isthing:
                if pred_class in stuff_memory_list:
                    segment_of_query[q] = stuff_memory_list[pred_class]
                    continue
                stuff_memory_list[pred_class] = current_segment_id + 1
            current_segment_id += 1
            segment_of_query[q] = current_segment_id
            segments_info.append({"id": current_segment_id, "isthing": bool(isthing), "category_id": pred_class})
    return segments_info, segment_of_query


def panoptic_argmax(mask_cls: torch.Tensor, mask_pred: torch.Tensor, geometry: Geometry, *, num_classes: int, object_mask_threshold: float):
    """The device half of ``panoptic_inference``: (``code`` int32 [H, W] = 2 q + (r_q >= 0) or -1, ``max_scores`` [Q], ``labels`` int32
    [Q], ``counts`` int32 [Q, 3]), all on the GPU; no copy to the host."""
    _check(mask_cls, mask_pred)
    dev = _require_cuda("sf_op_seg_panoptic_argmax", mask_cls, mask_pred)
    if mask_cls.shape[1] != num_classes + 1:
        raise ValueError(f"mask_cls has {mask_cls.shape[1]} columns, expected num_classes + 1 = {num_classes + 1}")
    padded, crop, out = _sizes(geometry)
    # the reference's max is over all C + 1 columns (a query whose best column is "no object" is dropped): a column of -inf behind them
    # has probability zero and is the one sf_op_vis_scores leaves out
    logits = _f32(mask_cls)
    widened = torch.cat([logits, logits.new_full((logits.shape[0], 1), float("-inf"))], dim=1)
    max_scores, labels, _ = vis_scores(widened)
    src = _f32(mask_pred)
    Q, h, w = src.shape
    code = torch.empty(out, dtype=torch.int32, device=dev)
    counts = torch.empty(Q, 3, dtype=torch.int32, device=dev)
    nat.launch(dev, nat.lib.sf_op_seg_panoptic_argmax, src.data_ptr(), max_scores.data_ptr(), labels.data_ptr(), Q, int(num_classes),
               float(object_mask_threshold), h, w, padded[0], padded[1], crop[0], crop[1], out[0], out[1], code.data_ptr(), counts.data_ptr())
    return code, max_scores, labels, counts


def panoptic_relabel(code: torch.Tensor, segment_of_query: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sf_op_seg_panoptic_relabel``: ``code`` int32 [H, W] and ``segment_of_query`` int32 [Q] on the GPU -> segment ids int32 [H, W];
    ``out`` may be ``code`` itself."""
    dev = _require_cuda("sf_op_seg_panoptic_relabel", code, segment_of_query)
    if code.dtype != torch.int32 or segment_of_query.dtype != torch.int32 or not code.is_contiguous() or not segment_of_query.is_contiguous():
        raise ValueError("code and segment_of_query must be contiguous int32 tensors")
    out = torch.empty_like(code) if out is None else out
    nat.launch(dev, nat.lib.sf_op_seg_panoptic_relabel, code.data_ptr(), segment_of_query.data_ptr(), segment_of_query.numel(), code.numel(),
               out.data_ptr())
    return out


@torch.no_grad()
def panoptic_inference(mask_cls: torch.Tensor, mask_pred: torch.Tensor, geometry: Geometry, *, num_classes: int, object_mask_threshold: float,
                       overlap_threshold: float, thing_classes: Iterable[int]) -> Tuple[torch.Tensor, List[Dict[str, Any]]]:
    """The reference's ``panoptic_inference`` with the resampling before it -> (``panoptic_seg`` int32 [H, W] on the GPU,
    ``segments_info``).  ``thing_classes``: the contiguous ids of the thing classes (the reference's
    ``metadata.thing_dataset_id_to_contiguous_id.values()``).  No kept query: a zero map and an empty list."""
    code, max_scores, labels, counts = panoptic_argmax(mask_cls, mask_pred, geometry, num_classes=num_classes, object_mask_threshold=object_mask_threshold)
    Q = labels.numel()
    host = _device_to_host(torch.cat([max_scores, labels.view(torch.float32), counts.view(torch.float32).flatten()]))
    segments_info, segment_of_query = panoptic_segments_host(host[:Q].tolist(), host[Q:2 * Q].view(torch.int32).tolist(),
                                                             host[2 * Q:].view(torch.int32).view(Q, 3).tolist(), num_classes=num_classes,
                                                             object_mask_threshold=object_mask_threshold, overlap_threshold=overlap_threshold,
                                                             thing_classes=thing_classes)
    table = torch.tensor(segment_of_query, dtype=torch.int32).to(code.device)
    return panoptic_relabel(code, table, out=code), segments_info


class SegmentationInstances:
    """What the reference's ``instance_inference`` returns in a detectron2 ``Instances``: ``image_size`` (H, W), ``pred_masks`` [K, H, W]
    (float 0 / 1 as the reference, or bool), ``pred_boxes`` [K, 4] zeros (as the reference), ``scores`` [K], ``pred_classes`` [K]."""

    def __init__(self, image_size: Tuple[int, int], pred_masks: torch.Tensor, pred_boxes: torch.Tensor, scores: torch.Tensor, pred_classes: torch.Tensor):
        self.image_size, self.pred_masks, self.pred_boxes, self.scores, self.pred_classes = image_size, pred_masks, pred_boxes, scores, pred_classes

    def __len__(self) -> int:
        return int(self.scores.shape[0])

    def __repr__(self) -> str:
        return f"SegmentationInstances(num_instances={len(self)}, image_size={self.image_size})"


@torch.no_grad()
def instance_inference(mask_cls: torch.Tensor, mask_pred: torch.Tensor, geometry: Geometry, *, num_classes: int, test_topk_per_image: int,
                       thing_classes: Optional[Iterable[int]] = None, as_bool: bool = False) -> SegmentationInstances:
    """The reference's ``instance_inference`` with the resampling before it: the top ``test_topk_per_image`` of the flattened [Q C] class
    scores (label = index % C, query = index // C), only thing classes when ``thing_classes`` is given (the reference's ``panoptic_on``
    branch), ``scores`` = class score x (sum of sigmoid over the mask's pixels) / (pixels + 1e-6).

    The result is SORTED by class score, descending (ties: the lower flattened index first, torch's rule); the reference takes
    ``topk(sorted=False)``, whose order is unspecified.  ``as_bool=True`` returns the masks as bool instead of the reference's float."""
    _check(mask_cls, mask_pred)
    dev = _require_cuda("instance_inference", mask_cls, mask_pred)
    if mask_cls.shape[1] != num_classes + 1:
        raise ValueError(f"mask_cls has {mask_cls.shape[1]} columns, expected num_classes + 1 = {num_classes + 1}")
    padded, crop, out = _sizes(geometry)
    scores = vis_scores(mask_cls, full=True)[2]
    top_scores, top = scores.flatten(0, 1).topk(min(int(test_topk_per_image), scores.numel()), sorted=True)
    labels = top % num_classes
    rows = top // num_classes
    if thing_classes is not None:
        keep = torch.isin(labels, torch.tensor(sorted(set(int(c) for c in thing_classes)), dtype=labels.dtype, device=dev))
        top_scores, labels, rows = top_scores[keep], labels[keep], rows[keep]
    K = int(rows.shape[0])
    boxes = torch.zeros(K, 4)
    if K == 0:
        masks = torch.zeros((0,) + out, dtype=torch.bool if as_bool else torch.float32, device=dev)
        return SegmentationInstances(out, masks, boxes, top_scores, labels)
    res = resample_masks(mask_pred, rows.to(torch.int32).view(K, 1), padded, crop, out)
    masks = res["masks"][:, 0]
    final = top_scores * (res["numerator"] / (res["denominator"].to(torch.float32) + 1e-6))
    return SegmentationInstances(out, masks if as_bool else masks.float(), boxes, final, labels)


class ImageSegmenter(nn.Module):
    """The eval branch of ``TimesformerMaskFormer.forward`` over the three native modules: normalise and pad the images to
    ``size_divisibility``, run backbone ([B, 1, 3, Hp, Wp]), pixel decoder and mask decoder, and per image the inference functions that
    are on.  Holds the modules and adds no parameters.  ``thing_classes`` stands for the reference's
    ``metadata.thing_dataset_id_to_contiguous_id.values()``."""

    def __init__(self, backbone: nn.Module, pixel_decoder: nn.Module, mask_decoder: nn.Module, *, num_queries: int, object_mask_threshold: float = 0.8,
                 overlap_threshold: float = 0.8, thing_classes: Iterable[int] = (), size_divisibility: int = 32,
                 sem_seg_postprocess_before_inference: bool = True, pixel_mean: Sequence[float] = (123.675, 116.28, 103.53),
                 pixel_std: Sequence[float] = (58.395, 57.12, 57.375), semantic_on: bool = True, panoptic_on: bool = False, instance_on: bool = False,
                 test_topk_per_image: int = 100):
        super().__init__()
        self.backbone, self.pixel_decoder, self.mask_decoder = backbone, pixel_decoder, mask_decoder
        self.num_queries, self.object_mask_threshold, self.overlap_threshold = int(num_queries), float(object_mask_threshold), float(overlap_threshold)
        self.thing_classes = tuple(int(c) for c in thing_classes)
        self.size_divisibility = int(size_divisibility)
        self.sem_seg_postprocess_before_inference = bool(sem_seg_postprocess_before_inference)
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.semantic_on, self.panoptic_on, self.instance_on = bool(semantic_on), bool(panoptic_on), bool(instance_on)
        self.test_topk_per_image = int(test_topk_per_image)
        if not self.semantic_on:
            assert self.sem_seg_postprocess_before_inference

    @property
    def device(self) -> torch.device:
        return self.pixel_mean.device

    def pre_process(self, batched_inputs: List[Dict[str, Any]]) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
        """The normalised images padded (bottom and right, zeros) to one size that ``size_divisibility`` divides, and each image's own size:
        ``VideoInstanceSegmenter.pre_process`` over the images as the frames of one clip (it reads ``device``, ``pixel_mean``, ``pixel_std``
        and ``size_divisibility``, which this module has under the same names)."""
        return VideoInstanceSegmenter.pre_process(self, [{"image": [x["image"] for x in batched_inputs]}])

    @torch.no_grad()
    def forward(self, batched_inputs: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """``batched_inputs``: per image ``{"image": (3, H, W), "height": .., "width": ..}`` (the last two default to the image's size).
        Returns per image a dict with ``"sem_seg"`` [C, height, width], ``"panoptic_seg"`` (int32 [height, width], segments_info) and
        ``"instances"``, whichever are on."""
        if self.training:
            raise NotImplementedError("ImageSegmenter is inference only: call .eval() (the criterion, SetCriterion, and the matcher, HungarianMatcher, "
                                      "are not part of the module)")
        batch, sizes = self.pre_process(batched_inputs)
        features = self.backbone(pixel_values=batch[:, None], output_attentions=False, output_hidden_states=True, return_dict=True)
        mask_features, _, multi_scale = self.pixel_decoder.forward_features(features)
        outputs = self.mask_decoder(multi_scale, mask_features)
        mask_cls_results, mask_pred_results = outputs["pred_logits"], outputs["pred_masks"]
        if mask_cls_results.shape[1] != self.num_queries:
            raise ValueError(f"the mask decoder returned {mask_cls_results.shape[1]} queries, num_queries = {self.num_queries}")
        num_classes = int(mask_cls_results.shape[-1]) - 1
        padded = (int(batch.shape[-2]), int(batch.shape[-1]))
        results: List[Dict[str, Any]] = []
        for mask_cls, mask_pred, per_image, image_size in zip(mask_cls_results, mask_pred_results, batched_inputs, sizes):
            out = (int(per_image.get("height", image_size[0])), int(per_image.get("width", image_size[1])))
            full = dict(padded=padded, crop=image_size, out=out)
            # without sem_seg_postprocess before inference the reference's panoptic and instance functions see the padded-size masks
            geometry = full if self.sem_seg_postprocess_before_inference else dict(padded=padded, crop=padded, out=padded)
            r: Dict[str, Any] = {}
            if self.semantic_on:
                r["sem_seg"] = semantic_inference(mask_cls, mask_pred, full, postprocess_before_inference=self.sem_seg_postprocess_before_inference)
            if self.panoptic_on:
                r["panoptic_seg"] = panoptic_inference(mask_cls, mask_pred, geometry, num_classes=num_classes, object_mask_threshold=self.object_mask_threshold,
                                                       overlap_threshold=self.overlap_threshold, thing_classes=self.thing_classes)
            if self.instance_on:
                r["instances"] = instance_inference(mask_cls, mask_pred, geometry, num_classes=num_classes, test_topk_per_image=self.test_topk_per_image,
                                                    thing_classes=self.thing_classes if self.panoptic_on else None)
            results.append(r)
        return results
