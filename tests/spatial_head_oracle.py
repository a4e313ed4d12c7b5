"""CPU restatement, in plain torch, of the spatial task head and the zero-shot classification head.

``TimesformerUniversalVideoInstanceSegmentationHead`` (reference ``models/modeling_timesformer_siglip.py:1729-1918``):
dense feature projection (``:1786-1795``), class sub-sampling above 100 classes (``:1844-1882``), bilinear upsample of
the patch logits to the mask size and per-pixel cross-entropy (``:1894-1916``).  ``TimesformerVideoClassificationHead``
(``:1704-1726``).  ``tools/make_golden_spatial_head.py`` pins both against the imported reference and records the
reference's tensors in ``tests/golden/f16_vis_head.npz``; the tests compare the HIP path against these functions.
Every function follows the dtype of its inputs: pass ``.double()`` tensors for the fp64 yardstick.
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

NUM_MAX_CLASSES = 100            # modeling:1826
PROJ_NAMES = ("w_v.weight", "w_v.bias", "v_proj.weight", "v_proj.bias", "head_layernorm.weight", "head_layernorm.bias",
              "head_mlp.fc1.weight", "head_mlp.fc1.bias", "head_mlp.fc2.weight", "head_mlp.fc2.bias")


def dense_projection(x: torch.Tensor, p: Dict[str, torch.Tensor], eps: float) -> torch.Tensor:
    """modeling:1786-1795 on rows [..., D]; ``p`` holds the ten tensors of ``PROJ_NAMES`` (erf GELU)."""
    y = F.linear(F.linear(x, p["w_v.weight"], p["w_v.bias"]), p["v_proj.weight"], p["v_proj.bias"])
    h = F.layer_norm(y, (y.shape[-1],), p["head_layernorm.weight"], p["head_layernorm.bias"], eps)
    h = F.linear(F.gelu(F.linear(h, p["head_mlp.fc1.weight"], p["head_mlp.fc1.bias"])), p["head_mlp.fc2.weight"], p["head_mlp.fc2.bias"])
    return y + h


def select_classes(table: torch.Tensor, mask_target: torch.Tensor, rng=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The label table and the remapped targets one clip trains against (modeling:1844-1892).

    At most 100 classes: the table as given, background (0) -> -1.  More: the positives present in the mask (ascending,
    ``torch.unique``) followed by ``random.sample`` negatives up to 100, rows RE-NORMALISED, every other target -> -1.
    ``rng``: a ``random.Random`` (default: the module-level generator the reference draws from)."""
    L = table.shape[0]
    if L <= NUM_MAX_CLASSES:
        t = mask_target.clone().long()
        return table, t.masked_fill(t == 0, -1)
    rng = rng or random
    uniq = torch.unique(mask_target)
    uniq = uniq[uniq > 0]
    num_neg = min(NUM_MAX_CLASSES - len(uniq), L - len(uniq))
    neg = list(set(range(L)) - set(uniq.cpu().numpy()))
    chosen = rng.sample(neg, num_neg)
    sel = torch.cat([uniq.long(), torch.tensor(chosen, dtype=torch.long, device=uniq.device)])
    rows = table[sel]
    rows = rows / rows.norm(p=2, dim=-1, keepdim=True)
    remap = torch.full((L,), -1, dtype=torch.long, device=mask_target.device)
    remap[sel] = torch.arange(len(sel), device=mask_target.device)
    t = mask_target.long()
    new = torch.where((t >= 0) & (t < L), remap[t.clamp(0, L - 1)], torch.full_like(t, -1))
    return rows, new


def mask_width(image_size: int, mask_size: Sequence[int]) -> int:
    """modeling:1895-1897."""
    target_h, target_w = int(mask_size[0]), int(mask_size[1])
    return int(target_w * (image_size / target_h))


def clip_mask_loss(x: torch.Tensor, table: torch.Tensor, target: torch.Tensor, logit_scale: torch.Tensor, logit_bias: torch.Tensor) -> torch.Tensor:
    """One clip: x [T, N, D] dense embeddings, table [L, D] as given, target int [T, H, W] (-1 = ignore) — modeling:1833-1836, 1885-1911."""
    T, N, _ = x.shape
    P = int(round(N ** 0.5))
    xn = x / x.norm(p=2, dim=-1, keepdim=True)
    z = torch.einsum("tpd,ld->tpl", xn, table.to(x.dtype)) * logit_scale.exp() + logit_bias
    z = z.reshape(T, P, P, -1).permute(0, 3, 1, 2)
    z = F.interpolate(z, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=False)
    if bool((target == -1).all()):
        return torch.zeros((), dtype=x.dtype, device=x.device)
    return F.cross_entropy(z, target.long(), ignore_index=-1)


def mask_loss(x: torch.Tensor, tables: List[torch.Tensor], targets: List[torch.Tensor], logit_scale, logit_bias) -> torch.Tensor:
    """x [B, T, N, D]; per-clip tables / targets already selected and remapped (what ``sf_mask_loss`` takes) — modeling:1914-1916."""
    return torch.stack([clip_mask_loss(x[i], tables[i], targets[i], logit_scale, logit_bias) for i in range(x.shape[0])]).mean()


def vis_head_loss(last_hidden_state: torch.Tensor, proj: Dict[str, torch.Tensor], eps: float, label_tables: Dict[str, torch.Tensor],
                  datasets: Sequence[str], mask_targets: Sequence[torch.Tensor], mask_sizes: Sequence[Sequence[int]], image_size: int,
                  logit_scale: torch.Tensor, logit_bias: torch.Tensor, rng=None) -> torch.Tensor:
    """The head's training forward (modeling:1810-1916): last_hidden_state [B, T, N, D] -> loss.  Each mask arrives at its
    training resolution [T, image_size, mask_width(image_size, mask_size)]."""
    dense = dense_projection(last_hidden_state, proj, eps)
    tables, targets = [], []
    for i, name in enumerate(datasets):
        tab, tgt = select_classes(label_tables[name].detach(), mask_targets[i], rng)
        assert tgt.shape[-2] == image_size and tgt.shape[-1] == mask_width(image_size, mask_sizes[i]), (tuple(tgt.shape), mask_sizes[i])
        tables.append(tab)
        targets.append(tgt)
    return mask_loss(dense, tables, targets, logit_scale, logit_bias)


def classification_loss(pooler: torch.Tensor, label_emb: torch.Tensor, labels: torch.Tensor, logit_scale: torch.Tensor,
                        logit_bias: torch.Tensor) -> torch.Tensor:
    """modeling:1704-1726: sigmoid loss of the LAST frame's pooled vector against one label table, summed over classes, mean over clips."""
    img = pooler[:, -1, :]
    img = img / img.norm(p=2, dim=-1, keepdim=True)
    logits = img @ label_emb.to(pooler.dtype).t() * logit_scale.exp() + logit_bias
    y = -torch.ones_like(logits)
    y[torch.arange(labels.shape[0]), labels.long()] = 1
    return -F.logsigmoid(y * logits).sum() / labels.shape[0]


def seeded_randn(seed: int, *shape) -> torch.Tensor:
    """Inputs of the fixtures and the GPU tests: CPU generator, fp32 (regenerated from the seed instead of stored)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def unit_rows(n: int, d: int, seed: int) -> torch.Tensor:
    e = seeded_randn(seed, n, d)
    return e / e.norm(dim=-1, keepdim=True)


def blocky_mask(seed: int, T: int, H: int, W: int, classes: Sequence[int], cells: int = 6) -> torch.Tensor:
    """Instance-like integer masks [T, H, W]: a coarse map of ``classes`` repeated up to the mask size."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.tensor(list(classes))[torch.randint(0, len(classes), (T, cells, cells), generator=g)]
    ys, xs = torch.arange(H) * cells // H, torch.arange(W) * cells // W
    return coarse[:, ys][:, :, xs].long().contiguous()


def bench_clip_inputs(seed: int = 1650, T: int = 16, P: int = 14, D: int = 768, L: int = 100, H: int = 224, W: int = 398):
    """One benchmark-sized clip (16 x 196 x 768 dense embeddings, 100 classes, a 224 x 398 mask of a 16:9 video):
    (x [T, N, D], table [L, D], target [T, H, W] with -1 = ignore on about a fifth of the cells)."""
    x = seeded_randn(seed, T, P * P, D)
    table = unit_rows(L, D, seed + 1)
    target = blocky_mask(seed + 2, T, H, W, [-1] * 25 + list(range(L)), cells=23)
    return x, table, target
