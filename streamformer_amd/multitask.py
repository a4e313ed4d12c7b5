"""The multitask wrapper of the pre-training step, as a torch module over the HIP encoder.

Mirror of ``StreamformerForMultiTaskingSigLIP`` (reference ``models/modeling_timesformer_siglip.py:1356-1536``) for the
three granularities of the pre-training — global: video-text retrieval (``TimesformerVideoRetrievalHead``, ``:2285-2351``) and
zero-shot classification (``TimesformerVideoClassificationHead``, ``:1651-1726``); temporal: per-frame localization
(``TimesformerUniversalLocalizationHead``, ``:2186-2282``) and caption-driven temporal grounding (``TimesformerTemporalGroundingHead``,
``:2354-2397``); spatial: video instance segmentation (``TimesformerUniversalVideoInstanceSegmentationHead``, ``:1729-1918``) and
referring segmentation (``TimesformerVideoContrastiveCrossEntropySegmentationHead``, ``:1921-2078``), both trained through
``last_hidden_state``:

    model = StreamformerForMultiTaskingSigLIP(config, {"TaskRetrieval": {}, "TaskLocalization": {"label2id": ...}})
    model.prepare_for_multi_tasks(); model.frozen_spatial(); model.cuda().train()
    losses, outputs = model(pixel_values, multi_task_input={"task_name": ..., "task_input": ...})
    losses[task].backward(); optimizer.step()                    # torch.optim over model.parameters()

Encoder forward / backward run in ``libstreamformer_hip.so`` behind one autograd node (``autograd.py``); the loss heads
are the HIP loss kernels (``sf_loss.hip``, ``sf_mask_loss.hip`` + ``sf_dense_head.hip``, ``sf_text_heads.hip``) behind a second one.
The SigLIP text tower (``:1365-1373``) is optional: given ``text_encoder`` (``text.SiglipTextModel``, the native tower) and
``text_tokenizer`` (the caller's tokenizer object), the caption heads take ``task_input["caption"]`` and the label-table heads build
their prompt-ensemble tables from ``prompt_templates``; without them captions / class prompts enter as feature tensors
(``task_input["text_features"]``, ``set_label_embeddings``), as before.  What is NOT here: two dispatches of the reference, which
raise ``NotImplementedError``: ``SSV2`` (the ``Kinetics`` head under a second name) and the naive localization head
(``THUMOS14`` / ``ActivityNet`` / ``FineAction`` / ``HACS``, ``:2081-2185``: window bookkeeping over pre-extracted features, not in
the shipped recipe).  With those two exceptions every task entry of the shipped recipe (``scripts/dataset_metadata/all.yaml``) builds.
"""
from __future__ import annotations

import copy
import math
import random
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from .configuration import StreamformerConfig
from .heads import DenseHeadProjection, DenseTextLogits, GroundingHead, LocalizationHead, MaskLossHead, RetrievalHead
from .modeling import TimesformerMultiTaskingModelSigLIP

RETRIEVAL_TASKS = ("MSRVTT", "WebVid", "TaskRetrieval")                                        # modeling:1401
LOCALIZATION_TASKS = ("THUMOS14Grounding", "ActivityNetGrounding", "FineActionGrounding", "HACSGrounding",
                      "TaskLocalization")                                                       # modeling:1384-1390
CLASSIFICATION_TASKS = ("Kinetics",)         # modeling:1380 also lists "SSV2" (same head): still refused here, tests/test_autograd_bridge.py
                                             # pins that refusal as its example of an unimplemented task type
VIS_TASKS = ("YoutubeVIS", "LVVIS", "COCOPseudoVIS", "TaskVIS")                                 # modeling:1416
GROUNDING_TASKS = ("CharadesSTA", "QVHighlights", "TaCoS", "TVSum", "ActivityNetCaptions", "DiDeMo", "QuerYD",
                   "TaskGrounding")                                                             # modeling:1404-1413
REFER_VOS_TASKS = ("MEVIS", "ReferYoutubeVOS", "RefCOCOPseudo", "TaskReferVOS")                 # modeling:1423-1428
NUM_MAX_CLASSES = 100                                                                           # modeling:1826


class _HeadLossFn(torch.autograd.Function):
    """loss = head.loss(pooler, ...) with the kernel's own gradients (d pooler, d logit_scale, d logit_bias) replayed."""

    @staticmethod
    def forward(ctx, pooler, logit_scale, logit_bias, run):
        loss, gp, gs = run(pooler.detach(), logit_scale.detach(), logit_bias.detach())
        ctx.save_for_backward(gp, gs)
        ctx.shapes = (logit_scale.shape, logit_bias.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        gp, gs = ctx.saved_tensors
        return gp * g, (gs[0] * g).reshape(ctx.shapes[0]), (gs[1] * g).reshape(ctx.shapes[1]), None


class _TaskHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.logit_scale = nn.Parameter(torch.tensor(math.log(10.0)))
        self.logit_bias = nn.Parameter(torch.tensor(-2.0))

    # the wrapper's frozen text tower and the caller's tokenizer (modeling:2207-2208, 2302-2303): plain attributes, NOT child modules —
    # the tower's parameters are listed once, under the wrapper, and a head's state_dict stays what it was
    _text_encoder = None
    _text_tokenizer = None

    def prepare_multi_task(self, text_encoder=None, text_tokenizer=None, logit_scale=None, logit_bias=None, vision_model=None):
        """modeling:2199-2205 / :2296-2301: every head deep-copies the wrapper's scale / bias pair and keeps the text tower."""
        if logit_scale is not None:
            self.logit_scale = copy.deepcopy(logit_scale)
        if logit_bias is not None:
            self.logit_bias = copy.deepcopy(logit_bias)
        object.__setattr__(self, "_text_encoder", text_encoder)
        object.__setattr__(self, "_text_tokenizer", text_tokenizer)

    def _caption_features(self, task_specific_input: dict, device) -> torch.Tensor:
        """``task_input["text_features"]`` [B, D] as given, or — with a text tower — ``task_input["caption"]`` (list of str) tokenised to
        64 tokens and encoded (modeling:2307-2316, 2378-2386, 1989-1998)."""
        if "text_features" in task_specific_input:
            return task_specific_input["text_features"].to(device)
        if "caption" not in task_specific_input:
            raise KeyError("task_input needs 'text_features' [B, D] or 'caption' (list of str)")
        if self._text_encoder is None or self._text_tokenizer is None:
            raise RuntimeError("task_input['caption'] needs the wrapper's text_encoder and text_tokenizer "
                               "(StreamformerForMultiTaskingSigLIP(..., text_encoder=, text_tokenizer=) + prepare_for_multi_tasks()); "
                               "without them pass task_input['text_features']")
        from .text import encode_captions
        return encode_captions(self._text_encoder, self._text_tokenizer, list(task_specific_input["caption"])).to(device)

    def _label_table(self, label2id: dict) -> Optional[torch.Tensor]:
        """The prompt-ensemble table of one label set (modeling:2207-2223), or None without a tower / templates."""
        templates = getattr(self, "prompt_templates", None)
        if self._text_encoder is None or self._text_tokenizer is None or not templates or not label2id:
            return None
        from .text import encode_label_prompts
        return encode_label_prompts(self._text_encoder, self._text_tokenizer, list(label2id.keys()), templates)

    def _build_dataset_tables(self) -> None:
        for name, l2i in self.label2id.items():
            if name not in self.dataset_label_embeddings and isinstance(l2i, dict):
                table = self._label_table(l2i)
                if table is not None:
                    self.dataset_label_embeddings[name] = table.detach()


class TimesformerVideoRetrievalHead(_TaskHead):
    """modeling:2285-2351.  ``task_input["text_features"]`` [B, D] stands in for ``encode_captions`` (:2307-2316);
    with torch.distributed initialised, every rank's captions are negatives (distributed SigLipLoss, :239-297)."""

    def __init__(self, config: Optional[StreamformerConfig] = None, gather_negatives: bool = True, process_group=None):
        super().__init__()
        self.config = config
        self.gather_negatives = gather_negatives
        self.group = process_group

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        pooler = task_head_input.pooler_output
        text = local_text = self._caption_features(task_specific_input, pooler.device)
        if not self.training:
            img = pooler[:, -1, :]
            return img / img.norm(p=2, dim=-1, keepdim=True), text / text.norm(p=2, dim=-1, keepdim=True)
        rank = 0
        if self.gather_negatives:
            from .parallel import all_gather_rows, world
            rank, ws = world(self.group)
            if ws > 1:
                text = all_gather_rows(text.contiguous(), group=self.group)
            else:
                rank = 0
        text = text.detach()              # frozen text tower (:1374-1375)

        def run(p, ls, lb):
            return RetrievalHead(ls, lb).loss(p, text, rank=rank)
        loss = _HeadLossFn.apply(pooler, self.logit_scale, self.logit_bias, run)
        with torch.no_grad():             # "logits for debugging" (:2346-2350): scale only, as in the reference
            img = pooler[:, -1, :]
            img = img / img.norm(p=2, dim=-1, keepdim=True)
            t = local_text
            logits = img @ (t / t.norm(p=2, dim=-1, keepdim=True)).t() * self.logit_scale.exp()
        return loss, logits


class TimesformerUniversalLocalizationHead(_TaskHead):
    """modeling:2186-2282.  ``label2id``: ``{dataset_name: {label: id}}``; the prompt-ensemble class embeddings of
    ``prepare_multi_task`` (:2207-2223, text tower) are supplied through :meth:`set_label_embeddings` ([L, D], unit norm)."""

    def __init__(self, config: Optional[StreamformerConfig] = None, label2id: Optional[dict] = None, prompt_templates=None):
        super().__init__()
        self.config = config
        self.label2id = label2id or {}
        self.prompt_templates = list(prompt_templates) if prompt_templates else None
        self.dataset_label_embeddings: Dict[str, torch.Tensor] = {}

    def set_label_embeddings(self, dataset_name: str, embeddings: torch.Tensor) -> None:
        self.dataset_label_embeddings[dataset_name] = embeddings.detach()

    def prepare_multi_task(self, text_encoder=None, text_tokenizer=None, logit_scale=None, logit_bias=None, vision_model=None):
        """With a text tower and ``prompt_templates``: every dataset's table that :meth:`set_label_embeddings` has not supplied."""
        super().prepare_multi_task(text_encoder, text_tokenizer, logit_scale, logit_bias, vision_model)
        self._build_dataset_tables()

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        pooler = task_head_input.pooler_output                     # [B, T, D]
        datasets = list(task_specific_input["dataset"])
        labels = task_specific_input["label"].to(pooler.device).long()
        B = pooler.shape[0]
        with torch.no_grad():
            img = pooler / pooler.norm(p=2, dim=-1, keepdim=True)
            all_logits = [img[i] @ self.dataset_label_embeddings[d].to(pooler.device).t() * self.logit_scale.exp() + self.logit_bias
                          for i, d in enumerate(datasets)]
        if not self.training:
            return all_logits
        total = None
        for name in dict.fromkeys(datasets):                        # clips grouped by dataset: one kernel launch per table
            idx = [i for i, d in enumerate(datasets) if d == name]
            emb = self.dataset_label_embeddings[name].to(pooler.device)
            whole = len(idx) == B
            p_g = pooler if whole else pooler[idx]
            lab_g = labels if whole else labels[idx]

            def run(p, ls, lb, emb=emb, lab_g=lab_g):
                return LocalizationHead(emb, ls, lb).loss(p, lab_g)
            part = _HeadLossFn.apply(p_g, self.logit_scale, self.logit_bias, run) * (len(idx) / B)
            total = part if total is None else total + part
        return total, all_logits


class TimesformerVideoClassificationHead(_TaskHead):
    """modeling:1651-1726 (task type ``Kinetics``; the reference's second name for it, ``SSV2``, is not dispatched yet): sigmoid loss of the LAST frame's pooled vector against one label
    table, ``-sum logsigmoid(+-logits) / B`` — the localization kernel on ``pooler[:, -1:, :]`` with labels [B, 1], so the
    gradient lands in the last frame's rows only.  In eval mode it returns the logits alone, the convention of the localization
    head here; the reference computes ``(loss, logits)`` in either mode (:1725-1726).  The prompt-ensemble class embeddings of ``prepare_multi_task`` (:1676-1684,
    text tower) are supplied through :meth:`set_label_embeddings` ([L, D], unit norm)."""

    def __init__(self, config: Optional[StreamformerConfig] = None, label2id: Optional[dict] = None, prompt_templates=None):
        super().__init__()
        self.config = config
        self.label2id = label2id or {}
        self.prompt_templates = list(prompt_templates) if prompt_templates else None
        self.label_embeddings: Optional[torch.Tensor] = None

    def set_label_embeddings(self, embeddings: torch.Tensor) -> None:
        self.label_embeddings = embeddings.detach()

    def prepare_multi_task(self, text_encoder=None, text_tokenizer=None, logit_scale=None, logit_bias=None, vision_model=None):
        """With a text tower and ``prompt_templates``: the class table, unless :meth:`set_label_embeddings` has supplied it."""
        super().prepare_multi_task(text_encoder, text_tokenizer, logit_scale, logit_bias, vision_model)
        if self.label_embeddings is None:
            table = self._label_table(self.label2id)
            if table is not None:
                self.label_embeddings = table.detach()

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        if self.label_embeddings is None:
            raise RuntimeError("set_label_embeddings([L, D]) first: the class prompts' text features are inputs here")
        pooler = task_head_input.pooler_output
        emb = self.label_embeddings.to(pooler.device)
        labels = task_specific_input["label"].to(pooler.device).long()
        last = pooler[:, -1:, :]
        with torch.no_grad():
            img = last[:, 0] / last[:, 0].norm(p=2, dim=-1, keepdim=True)
            logits = img @ emb.t() * self.logit_scale.exp() + self.logit_bias
        if not self.training:
            return logits

        def run(p, ls, lb):
            return LocalizationHead(emb, ls, lb).loss(p, labels.reshape(-1, 1))
        return _HeadLossFn.apply(last, self.logit_scale, self.logit_bias, run), logits


class TimesformerTemporalGroundingHead(_TaskHead):
    """modeling:2354-2397 (task types ``CharadesSTA`` / ``QVHighlights`` / ``TaCoS`` / ``TVSum`` / ``ActivityNetCaptions`` / ``DiDeMo`` /
    ``QuerYD`` / ``TaskGrounding``): the one task where a caption supervises EVERY frame — sigmoid loss of each frame's pooled vector
    against the clip's own caption, ``-sum logsigmoid(y * logits) / B`` with ``y = -1`` where ``label`` is 0 (``sf_grounding_loss``).
    ``task_input["text_features"]`` [B, D] stands in for the tokenizer + text tower (:2378-2386), ``task_input["label"]`` is [B, T].
    Local captions only: the reference gathers nothing across ranks for this head.  In eval mode it returns the logits [B, T] alone,
    the convention of the localization / classification heads here; the reference computes ``(loss, logits)`` in either mode (:2396-2397)."""

    def __init__(self, config: Optional[StreamformerConfig] = None):
        super().__init__()
        self.config = config

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        pooler = task_head_input.pooler_output                     # [B, T, D]
        text = self._caption_features(task_specific_input, pooler.device).detach()      # frozen text tower (:1372-1373)
        if not self.training:
            with torch.no_grad():
                return GroundingHead(self.logit_scale, self.logit_bias).logits(pooler, text)
        labels = task_specific_input["label"].to(pooler.device)
        kept = {}

        def run(p, ls, lb):
            loss, gp, gs, kept["logits"] = GroundingHead(ls, lb).loss(p, text, labels, return_logits=True)
            return loss, gp, gs
        loss = _HeadLossFn.apply(pooler, self.logit_scale, self.logit_bias, run)
        return loss, kept["logits"]


def select_vis_classes(table: torch.Tensor, mask_target: torch.Tensor, rng=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The label rows and remapped targets one clip trains against (modeling:1844-1892; host logic).  At most 100 classes: the table
    as given (NOT re-normalised), background 0 -> -1.  More: the positives present in the mask (ascending) followed by
    ``random.sample`` negatives up to 100, targets remapped, everything else -> -1, and only here the selected rows are
    re-normalised.  ``rng``: a ``random.Random``; default the module-level generator the reference draws from, so
    ``random.seed(k)`` replays its draw."""
    L = table.shape[0]
    t = mask_target.long()
    if L <= NUM_MAX_CLASSES:
        return table, t.masked_fill(t == 0, -1)
    uniq = torch.unique(t)
    uniq = uniq[uniq > 0]
    num_neg = min(NUM_MAX_CLASSES - len(uniq), L - len(uniq))
    neg = list(set(range(L)) - set(uniq.cpu().numpy()))
    chosen = (rng or random).sample(neg, num_neg)
    sel = torch.cat([uniq, torch.tensor(chosen, dtype=torch.long, device=uniq.device)])
    rows = table[sel.to(table.device)]
    rows = rows / rows.norm(p=2, dim=-1, keepdim=True)
    remap = torch.full((L,), -1, dtype=torch.long, device=t.device)
    remap[sel] = torch.arange(len(sel), device=t.device)
    return rows, torch.where((t >= 0) & (t < L), remap[t.clamp(0, L - 1)], torch.full_like(t, -1))


class _VisLossFn(torch.autograd.Function):
    """loss = mask_loss(dense_projection(last_hidden_state)): one node over the dense projection (``sf_dense_head_*``) and the
    fused mask loss (``sf_mask_loss``).  The loss is a scalar, so the whole backward runs in forward (the projection's saved
    activations live only for this call) and backward() scales the stored gradients."""

    @staticmethod
    def forward(ctx, proj, tables, targets, lhs, logit_scale, logit_bias, *params):
        dense = proj.forward(lhs.detach(), [p.detach() for p in params])
        loss, g_dense, g_scalars = MaskLossHead(logit_scale.detach(), logit_bias.detach()).loss(dense, tables, targets)
        d_lhs, grads = proj.backward(g_dense)
        ctx.save_for_backward(d_lhs, g_scalars, *grads)
        ctx.shapes = (logit_scale.shape, logit_bias.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_lhs, gs, *grads = ctx.saved_tensors
        return (None, None, None, d_lhs * g, (gs[0] * g).reshape(ctx.shapes[0]), (gs[1] * g).reshape(ctx.shapes[1])) + tuple(
            pg * g for pg in grads)


class _HeadMlp(nn.Module):
    def __init__(self, D: int, I: int):
        super().__init__()
        self.fc1 = nn.Linear(D, I)
        self.fc2 = nn.Linear(I, D)


class _DenseProjectionHead(_TaskHead):
    """What the two segmentation heads share (modeling:1764-1795 and, the same lines again, :1940-1971): the pooling head registered as
    the child ``head`` and the head's own copies of its value projection, out_proj, layernorm and mlp, applied to every patch token
    by ``DenseHeadProjection``."""

    def __init__(self, config: StreamformerConfig, label2id: Optional[dict] = None, head: Optional[nn.Module] = None,
                 prompt_templates=None):
        super().__init__()
        self.config = config
        self.label2id = label2id or {}
        self.prompt_templates = list(prompt_templates) if prompt_templates else None
        if head is not None:
            self.head = head
        if config.hidden_act != "gelu":
            raise NotImplementedError(f"hidden_act={config.hidden_act!r}: the dense projection's training kernels implement the erf GELU")
        self._proj = DenseHeadProjection(config.layer_norm_eps)

    def _build_projection(self) -> None:
        D, I = self.config.hidden_size, self.config.intermediate_size
        self.w_v = nn.Linear(D, D, bias=True)
        self.v_proj = nn.Linear(D, D, bias=True)
        self.head_layernorm = nn.LayerNorm(D, eps=self.config.layer_norm_eps)
        self.head_mlp = _HeadMlp(D, I)

    def projection_parameters(self):
        return [self.w_v.weight, self.w_v.bias, self.v_proj.weight, self.v_proj.bias, self.head_layernorm.weight, self.head_layernorm.bias,
                self.head_mlp.fc1.weight, self.head_mlp.fc1.bias, self.head_mlp.fc2.weight, self.head_mlp.fc2.bias]

    def _copy_projection(self, vision_model) -> None:
        D = self.config.hidden_size
        src = dict(vision_model.head.named_parameters())           # modeling:1764-1779: deep copies of the pooling head's tensors
        with torch.no_grad():
            for dst, val in zip(self.projection_parameters(),
                                (src["attention.in_proj_weight"][2 * D:, :], src["attention.in_proj_bias"][2 * D:], src["attention.out_proj.weight"],
                                 src["attention.out_proj.bias"], src["layernorm.weight"], src["layernorm.bias"], src["mlp.fc1.weight"],
                                 src["mlp.fc1.bias"], src["mlp.fc2.weight"], src["mlp.fc2.bias"])):
                dst.data = val.detach().clone().to(dst.dtype)

    def _check_mask(self, i: int, target: torch.Tensor, mask_size) -> None:
        """modeling:1895-1897 / :2029-2030: masks arrive at their training resolution, height = image size, width scaled with it."""
        H = self.config.image_size
        target_h, target_w = mask_size
        new_w = int(int(target_w) * (H / int(target_h)))
        if target.shape[-2] != H or target.shape[-1] != new_w:
            raise ValueError(f"clip {i}: mask_target must arrive at its training resolution [T, {H}, {new_w}] "
                             f"(mask_size {tuple(int(v) for v in mask_size)}), got {tuple(target.shape)}")


class TimesformerUniversalVideoInstanceSegmentationHead(_DenseProjectionHead):
    """modeling:1729-1918 (task types ``YoutubeVIS`` / ``LVVIS`` / ``COCOPseudoVIS`` / ``TaskVIS``): the spatial task.  All patch
    tokens go through the head's own copies of the pooling head's value projection, out_proj, layernorm and mlp
    (``w_v``, ``v_proj``, ``head_layernorm``, ``head_mlp``; :1764-1779, :1786-1795), their cosine logits against a per-dataset
    label table are upsampled to the mask size and trained with a per-pixel cross-entropy (:1829-1916).

    Parameters, as in the reference: ``logit_scale``, ``logit_bias``, then — when ``head`` (the encoder's pooling head) is given,
    which the wrapper does — that module registered as the child ``head`` (SHARED tensors: under the wrapper they are listed once,
    as ``timesformer.head.*``, by ``named_parameters()`` and twice by ``state_dict()``), then ``w_v.*``, ``v_proj.*``,
    ``head_layernorm.*``, ``head_mlp.fc1.*``, ``head_mlp.fc2.*``.  The ten projection tensors TRAIN: the reference's
    ``requires_grad = False`` lines (:1781-1784) set an attribute on modules and freeze nothing.
    ``label2id``: ``{dataset_name: {label: id}}``; the class embeddings of ``prepare_multi_task`` (:1748-1762, text tower) come
    through :meth:`set_label_embeddings`."""

    def __init__(self, config: StreamformerConfig, label2id: Optional[dict] = None, head: Optional[nn.Module] = None,
                 prompt_templates=None):
        super().__init__(config, label2id, head, prompt_templates)
        self._build_projection()
        self.dataset_label_embeddings: Dict[str, torch.Tensor] = {}
        self.class_rng: Optional[random.Random] = None      # None: the module-level `random`, as the reference

    def prepare_multi_task(self, text_encoder=None, text_tokenizer=None, logit_scale=None, logit_bias=None, vision_model=None):
        super().prepare_multi_task(text_encoder, text_tokenizer, logit_scale, logit_bias, vision_model)
        if vision_model is not None:
            self._copy_projection(vision_model)
        self._build_dataset_tables()            # modeling:1748-1762, when a text tower and prompt_templates are given

    def set_label_embeddings(self, dataset_name: str, embeddings: torch.Tensor) -> None:
        self.dataset_label_embeddings[dataset_name] = embeddings.detach()

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        if not self.training:
            return None                                             # modeling:1914-1918: the head has no evaluation output
        lhs = task_head_input.last_hidden_state                    # [B, T, N, D]
        B = lhs.shape[0]
        tables, targets = [], []
        for i in range(B):
            name = task_specific_input["dataset"][i]
            tab, tgt = select_vis_classes(self.dataset_label_embeddings[name].to(lhs.device), task_specific_input["mask_target"][i].to(lhs.device),
                                          self.class_rng)
            self._check_mask(i, tgt, task_specific_input["mask_size"][i])
            tables.append(tab)
            targets.append(tgt)
        loss = _VisLossFn.apply(self._proj, tables, targets, lhs, self.logit_scale, self.logit_bias, *self.projection_parameters())
        return loss, None


def refer_mask_targets(mask_targets, rank: int, batch: int):
    """modeling:2045-2060: clip i trains against the WHOLE gathered caption table; its pixels equal to 1 get the class
    ``rank * batch + i`` (this clip's own caption), every other pixel -1 (ignored)."""
    out = []
    for i, m in enumerate(mask_targets):
        m = m.long()
        out.append(torch.where(m == 1, torch.full_like(m, rank * batch + i), torch.full_like(m, -1)))
    return out


class TimesformerVideoContrastiveCrossEntropySegmentationHead(_DenseProjectionHead):
    """modeling:1921-2078 (task types ``MEVIS`` / ``ReferYoutubeVOS`` / ``RefCOCOPseudo`` / ``TaskReferVOS``): referring segmentation,
    the per-pixel counterpart of the grounding head.  The dense projection and the upsample + per-pixel cross-entropy are the VIS
    head's (``sf_dense_head_*``, ``sf_mask_loss``); the class table is the captions of the whole (gathered) batch.

    ``task_input["text_features"]`` [B, D] stands in for the tokenizer + text tower (:1989-1998).  With ``torch.distributed``
    initialised the rows are all-gathered over ranks into [W * B, D] (:2000-2002), normalised row-wise and detached.  Clip ``i``
    trains against that whole table with target ``rank * B + i`` where ``mask_target[i] == 1`` and -1 elsewhere; the masks arrive at
    height ``config.image_size`` and width ``int(target_w * (image_size / target_h))`` (:2029-2030 — the reference hard-codes 224 and
    a 14 x 14 patch grid; here the grid is ``sqrt(N)`` and the height the configured image size, as in the VIS head).  The loss is the
    mean over clips of the per-clip mean cross-entropy over non-ignored pixels.  A clip whose mask has no pixel equal to 1 makes the
    reference's ``cross_entropy`` return NaN; here it contributes loss 0 and no gradient and is still counted in the mean (the
    convention of ``sf_mask_loss``).  At most 128 gathered captions (the mask loss's class capacity).

    Training returns ``(loss, None)``: the reference also hands back its [B, T, N, W * B] similarity tensor, which nothing consumes.
    Evaluation returns the dense caption-to-patch logits against the LOCAL captions, [B, T, N, B] (:2016-2018, no gather), from
    ``sf_dense_text_logits``; the dense projection's saved activations are released right after.

    Parameters, as in the reference: ``logit_scale``, ``logit_bias``, the shared pooling head as the child ``head``, and — created by
    :meth:`prepare_multi_task`, not by the constructor (:1940-1955) — ``w_v.*``, ``v_proj.*``, ``head_layernorm.*``, ``head_mlp.fc1.*``,
    ``head_mlp.fc2.*``; all ten train (:1957-1960 set an attribute on modules and freeze nothing)."""

    def __init__(self, config: StreamformerConfig, label2id: Optional[dict] = None, head: Optional[nn.Module] = None, process_group=None):
        super().__init__(config, label2id, head)
        self.group = process_group

    def prepare_multi_task(self, text_encoder=None, text_tokenizer=None, logit_scale=None, logit_bias=None, vision_model=None):
        super().prepare_multi_task(text_encoder, text_tokenizer, logit_scale, logit_bias, vision_model)
        if vision_model is None:
            return
        if not hasattr(self, "w_v"):          # a second call refills the SAME tensors: an optimizer built in between keeps training them
            self._build_projection()          # (the reference creates new modules on every call and orphans the optimizer's)
        self._copy_projection(vision_model)

    def forward(self, task_head_input, task_specific_input: Optional[dict] = None):
        if not hasattr(self, "w_v"):
            raise RuntimeError("prepare_multi_task(vision_model=...) first: it creates this head's dense projection (modeling:1940-1955)")
        lhs = task_head_input.last_hidden_state                    # [B, T, N, D]
        B, T, N, D = lhs.shape
        text = self._caption_features(task_specific_input, lhs.device).detach().float()      # frozen text tower (:1372-1373)
        if tuple(text.shape) != (B, D):
            raise ValueError(f"text_features must be [{B}, {D}] (one caption per clip), got {tuple(text.shape)}")
        if not self.training:
            with torch.no_grad():
                try:
                    dense = self._proj.forward(lhs, self.projection_parameters())
                    return DenseTextLogits(self.logit_scale, self.logit_bias).forward(dense, text)
                finally:
                    self._proj.release()                           # ~1 GB of saved activations at 8 clips: no backward follows
        from .parallel import all_gather_rows, world
        rank, ws = world(self.group)
        if ws > 1:
            text = all_gather_rows(text.contiguous(), group=self.group)
        else:
            rank = 0
        table = text / text.norm(p=2, dim=-1, keepdim=True)
        masks = [m.to(lhs.device) for m in task_specific_input["mask_target"]]
        if len(masks) != B:
            raise ValueError(f"{B} clips need {B} masks, got {len(masks)}")
        for i, m in enumerate(masks):
            self._check_mask(i, m, task_specific_input["mask_size"][i])
        targets = refer_mask_targets(masks, rank, B)
        loss = _VisLossFn.apply(self._proj, [table] * B, targets, lhs, self.logit_scale, self.logit_bias, *self.projection_parameters())
        return loss, None


class StreamformerForMultiTaskingSigLIP(nn.Module):
    """modeling:1356-1536: ``timesformer`` + per-task heads, one task per call.  ``text_encoder`` (``text.SiglipTextModel``, frozen;
    registered as the child ``text_encoder`` like the reference's, :1365-1375) and ``text_tokenizer`` (the caller's tokenizer) are
    optional and go together; ``multi_task_config[task]["prompt_templates"]`` (format strings with one ``{}``) lets the label-table
    heads build their class tables from them."""

    def __init__(self, config: StreamformerConfig, multi_task_config: Optional[dict] = None, compute_dtype="fp32",
                 text_encoder=None, text_tokenizer=None):
        super().__init__()
        self.config = config
        if (text_encoder is None) != (text_tokenizer is None):
            raise ValueError("text_encoder and text_tokenizer go together: the heads tokenise captions before they encode them")
        if text_encoder is not None:
            self.text_encoder = text_encoder
            for p in self.text_encoder.parameters():             # modeling:1374-1375
                p.requires_grad = False
        self.text_tokenizer = text_tokenizer
        self.timesformer = TimesformerMultiTaskingModelSigLIP(config, compute_dtype=compute_dtype)
        self.logit_scale = nn.Parameter(torch.log(torch.tensor(10.0)))
        self.logit_bias = nn.Parameter(torch.tensor(-2.0))
        self.task_heads = nn.ModuleDict()
        self.task_types = list(multi_task_config.keys()) if multi_task_config else []
        for task_type in self.task_types:
            if task_type in LOCALIZATION_TASKS:
                self.task_heads[task_type] = TimesformerUniversalLocalizationHead(config, (multi_task_config[task_type] or {}).get("label2id"),
                                                                                  (multi_task_config[task_type] or {}).get("prompt_templates"))
            elif task_type in RETRIEVAL_TASKS:
                self.task_heads[task_type] = TimesformerVideoRetrievalHead(config)
            elif task_type in CLASSIFICATION_TASKS:
                self.task_heads[task_type] = TimesformerVideoClassificationHead(config, (multi_task_config[task_type] or {}).get("label2id"),
                                                                                (multi_task_config[task_type] or {}).get("prompt_templates"))
            elif task_type in VIS_TASKS:
                self.task_heads[task_type] = TimesformerUniversalVideoInstanceSegmentationHead(
                    config, (multi_task_config[task_type] or {}).get("label2id"), self.timesformer.head,
                    (multi_task_config[task_type] or {}).get("prompt_templates"))
            elif task_type in GROUNDING_TASKS:
                self.task_heads[task_type] = TimesformerTemporalGroundingHead(config)
            elif task_type in REFER_VOS_TASKS:
                self.task_heads[task_type] = TimesformerVideoContrastiveCrossEntropySegmentationHead(
                    config, (multi_task_config[task_type] or {}).get("label2id"), self.timesformer.head)
            else:
                raise NotImplementedError(f"Task type {task_type} not implemented (this build covers the retrieval, localization, classification, "
                                          "temporal grounding, video instance segmentation and referring segmentation heads; still refused: "
                                          "SSV2, and the naive localization head of THUMOS14 / ActivityNet / FineAction / HACS)")
        if config.add_lora_spatial:
            self.add_lora_spatial()
        self.train()                      # an nn.Module is born in train mode; the encoder child alone is born in eval mode

    def frozen_backbone(self):
        for p in self.timesformer.parameters():
            p.requires_grad = False
        print("Backbone frozen")

    def prepare_for_multi_tasks(self):
        for head in self.task_heads.values():
            head.prepare_multi_task(getattr(self, "text_encoder", None), self.text_tokenizer, self.logit_scale, self.logit_bias, self.timesformer)

    def add_lora_spatial(self):
        """modeling:1448-1459: rank-32 factors on every spatial qkv / output.dense; `_add_lora` freezes the base qkv / dense
        (modeling:519-522)."""
        self.timesformer.add_lora_spatial()

    def frozen_spatial(self):
        """modeling:1461-1476: spatial ``attention.qkv`` AND ``output.dense`` (weight + bias) stop training."""
        for i in range(self.config.num_hidden_layers):
            for n in ("attention.attention.qkv", "attention.output.dense"):
                for leaf in ("weight", "bias"):
                    p = self.timesformer._named.get(f"encoder.layer.{i}.{n}.{leaf}")
                    if p is not None:
                        p.requires_grad = False

    def forward(self, pixel_values=None, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                multi_task_input: Optional[dict] = None):
        c = self.config
        if pixel_values.dim() != 5:           # modeling:1497-1503 flattens to clips of config.num_frames; 5-D input keeps its T
            pixel_values = pixel_values.reshape(-1, c.num_frames, 3, c.image_size, c.image_size)
        backbone_outputs = self.timesformer(pixel_values, output_attentions=output_attentions,
                                            output_hidden_states=output_hidden_states, return_dict=True)
        task_name = multi_task_input["task_name"]           # one task at a time (modeling:1514)
        if not self.training:
            return {task_name: self.task_heads[task_name](backbone_outputs, multi_task_input["task_input"])}
        loss, out = self.task_heads[task_name](backbone_outputs, multi_task_input["task_input"])
        return {task_name: loss}, {task_name: out}

    @torch.no_grad()
    def forward_features(self, pixel_values, pooling_method="mean"):
        return self.timesformer.forward_features(pixel_values, pooling_method)
