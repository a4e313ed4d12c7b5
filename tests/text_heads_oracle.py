"""CPU restatement, in plain torch, of the two caption-driven heads.

``TimesformerTemporalGroundingHead`` (reference ``models/modeling_timesformer_siglip.py:2354-2397``): one caption per clip against
every frame's pooled vector, sigmoid loss.  ``TimesformerVideoContrastiveCrossEntropySegmentationHead`` (``:1921-2078``): the dense
projection and upsample + per-pixel cross-entropy of the spatial head (``tests/spatial_head_oracle.py``) with the gathered,
normalised captions as the class table.  ``tools/make_golden_text_heads.py`` pins both against the imported reference and records
the reference's tensors in ``tests/golden/f17_text_heads.npz``; the tests compare the HIP path against these functions.
Every function follows the dtype of its inputs: pass ``.double()`` tensors for the fp64 yardstick.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

from tests import spatial_head_oracle as S


def grounding_logits(pooler: torch.Tensor, text: torch.Tensor, logit_scale: torch.Tensor, logit_bias: torch.Tensor) -> torch.Tensor:
    """modeling:2388-2392: pooler [B, T, D], text [B, D] (one caption per clip) -> logits [B, T]."""
    img = pooler / pooler.norm(p=2, dim=-1, keepdim=True)
    txt = text.to(pooler.dtype)
    txt = txt / txt.norm(p=2, dim=-1, keepdim=True)
    return torch.einsum("btd,bd->bt", img, txt) * logit_scale.exp() + logit_bias


def grounding_loss(pooler: torch.Tensor, text: torch.Tensor, labels: torch.Tensor, logit_scale: torch.Tensor,
                   logit_bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """modeling:2394-2397: labels [B, T] numbers, 0 -> -1 (``masked_fill``), everything else as given; -> (loss, logits)."""
    logits = grounding_logits(pooler, text, logit_scale, logit_bias)
    y = labels.masked_fill(labels == 0, -1).to(logits.dtype)
    return -F.logsigmoid(y * logits).sum() / logits.shape[0], logits


def dense_text_logits(x: torch.Tensor, text: torch.Tensor, logit_scale: torch.Tensor, logit_bias: torch.Tensor) -> torch.Tensor:
    """modeling:2004-2014: x [..., D] dense embeddings, text [n, D] un-normalised -> [..., n]."""
    xn = x / x.norm(p=2, dim=-1, keepdim=True)
    t = text.to(x.dtype)
    t = t / t.norm(p=2, dim=-1, keepdim=True)
    return xn @ t.t() * logit_scale.exp() + logit_bias


def refer_targets(mask_targets: Sequence[torch.Tensor], rank: int, batch: int) -> List[torch.Tensor]:
    """modeling:2045-2060: pixels equal to 1 -> the clip's own caption ``rank * batch + i``; every other pixel -> -1 (ignored)."""
    out = []
    for i, m in enumerate(mask_targets):
        t = -torch.ones_like(m, dtype=torch.long)
        t[m.long() == 1] = rank * batch + i
        out.append(t)
    return out


def refer_table(text_all: torch.Tensor) -> torch.Tensor:
    """modeling:2007-2009: the gathered captions [W * B, D], normalised row-wise (no gradient: frozen text tower)."""
    return (text_all / text_all.norm(p=2, dim=-1, keepdim=True)).detach()


def refer_head_loss(last_hidden_state: torch.Tensor, proj: Dict[str, torch.Tensor], eps: float, text_all: torch.Tensor, rank: int,
                    mask_targets: Sequence[torch.Tensor], mask_sizes: Sequence[Sequence[int]], image_size: int,
                    logit_scale: torch.Tensor, logit_bias: torch.Tensor) -> torch.Tensor:
    """The head's training forward (modeling:1976-2078): last_hidden_state [B, T, N, D], text_all [W * B, D] (this rank's rows at
    ``rank * B``) -> loss.  Each mask arrives at [T, image_size, mask_width(image_size, mask_size)]."""
    B = last_hidden_state.shape[0]
    dense = S.dense_projection(last_hidden_state, proj, eps)
    for m, size in zip(mask_targets, mask_sizes):
        assert m.shape[-2] == image_size and m.shape[-1] == S.mask_width(image_size, size), (tuple(m.shape), size)
    table = refer_table(text_all).to(dense.dtype)
    return S.mask_loss(dense, [table] * B, refer_targets(mask_targets, rank, B), logit_scale, logit_bias)


def refer_head_logits(last_hidden_state: torch.Tensor, proj: Dict[str, torch.Tensor], eps: float, text_local: torch.Tensor,
                      logit_scale: torch.Tensor, logit_bias: torch.Tensor) -> torch.Tensor:
    """The head's evaluation forward (modeling:2004-2018): logits against the LOCAL captions, [B, T, N, B]."""
    return dense_text_logits(S.dense_projection(last_hidden_state, proj, eps), text_local, logit_scale, logit_bias)


def bench_grounding_inputs(seed: int = 1750, B: int = 8, T: int = 16, D: int = 768):
    """The benchmark shape of the grounding loss: (pooler [B, T, D], text [B, D], labels [B, T] in {0, 1})."""
    g = torch.Generator().manual_seed(seed + 2)
    return S.seeded_randn(seed, B, T, D), S.seeded_randn(seed + 1, B, D), torch.randint(0, 2, (B, T), generator=g).float()


def bench_dense_inputs(seed: int = 1760, M: int = 8 * 16 * 196, D: int = 768, n: int = 8):
    """The benchmark shape of the dense text logits: (x [M, D], text [n, D])."""
    return S.seeded_randn(seed, M, D), S.seeded_randn(seed + 1, n, D)


# edge shapes of the dense text logits kernel, name -> (seed, M, D, n): one caption, the capacity (two LDS passes at D = 768), row counts
# that are not a multiple of a workgroup's 8 rows, feature widths that are not a multiple of 256
EDGE_DENSE_SHAPES = {"n1": (1770, 1000, 128, 1), "n64": (1772, 515, 768, 64), "ragged": (1774, 1003, 192, 5), "wide": (1776, 77, 1152, 17)}
