"""Helper of the connector tests (not a test file): the video-LLM connector restated in torch in the REFERENCE's order, at a chosen
precision.  Nothing here imports the package under test or the reference.

    projector : Linear (+ erf GELU + Linear ...) on every patch token                    (mm_projector)
    pool      : per frame, over the P x P grid of projected tokens                       (get_2dPool)
                  bilinear  P' = ceil(P / s); src = (dst + 0.5) P / P' - 0.5 clamped below at 0, i0 = floor(src), i1 = min(i0 + 1, P - 1),
                            weights (1 - lambda, lambda) with lambda = src - i0, separable in y and x   (align_corners=False, no antialias)
                  average   P' = floor(P / s); the mean of each s x s window, trailing rows / columns dropped
                  max       the same windows, their maximum
    newline   : grid = one image_newline row after every grid row of every frame, frame = one after every frame, one_token = one after
                the last frame (only with "unpad" in mm_patch_merge_type), no_token / the flat merge type = none

The pools are written as explicit tap matrices (not as calls of F.interpolate / F.avg_pool2d): the fixture ``tests/golden/
f19_connector.npz`` holds the outputs of the reference's own code, and the tap rules above are what this restatement is checked against.

``forward(..., dtype=torch.float64)`` is the reference of the GPU tests; ``dtype=torch.float32`` with ``bf16_operands="x3"`` / ``True`` are
the precision floors of the accurate and the bf16 mode (operands of every Linear as hi + lo bf16 planes with the lo * lo product dropped /
rounded to bf16; fp32 accumulation; everything else fp32), stated once in ``tests/oracle_ops.py``.
"""
import math
import os

import numpy as np
import torch

from tests.oracle_ops import activation, operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_connector.npz")

D_IN, D_OUT, FRAMES = 64, 128, 2
WEIGHT_SEEDS = {"mlp2x_gelu": 1901, "linear": 1902}
# name -> (projector, pool mode, P, newline position): all three modes, both grids (5: odd, clamped edge / dropped row; 6: even), the four
# newline positions, both projector types
CASES = {
    "mlp_bil_p5_grid": ("mlp2x_gelu", "bilinear", 5, "grid"),
    "mlp_bil_p6_frame": ("mlp2x_gelu", "bilinear", 6, "frame"),
    "mlp_avg_p5_one": ("mlp2x_gelu", "average", 5, "one_token"),
    "mlp_avg_p6_grid": ("mlp2x_gelu", "average", 6, "grid"),
    "mlp_max_p5_none": ("mlp2x_gelu", "max", 5, "no_token"),
    "lin_max_p6_frame": ("linear", "max", 6, "frame"),
    "lin_bil_p6_one": ("linear", "bilinear", 6, "one_token"),
    "lin_avg_p5_none": ("linear", "average", 5, "no_token"),
}


def case_config(name, d_in=D_IN, d_out=D_OUT, stride=2):
    proj, mode, _, newline = CASES[name]
    return make_config(proj, mode, newline, d_in, d_out, stride)


def make_config(proj="mlp2x_gelu", mode="bilinear", newline="grid", d_in=D_IN, d_out=D_OUT, stride=2, merge="spatial_unpad"):
    return dict(mm_projector_type=proj, mm_hidden_size=d_in, hidden_size=d_out, mm_spatial_pool_stride=stride, mm_spatial_pool_mode=mode,
                mm_newline_position=newline, mm_patch_merge_type=merge)


def projector_depth(projector_type):
    if projector_type == "linear":
        return 1
    if projector_type == "identity":
        return 0
    return int(projector_type[len("mlp"):projector_type.index("x_gelu")])


def linear_keys(projector_type):
    """Prefixes of the Linears under the reference builder's names: ``mm_projector.`` (linear), ``mm_projector.{0,2,...}.`` (nn.Sequential)."""
    n = projector_depth(projector_type)
    return ["mm_projector."] if projector_type == "linear" else [f"mm_projector.{2 * i}." for i in range(n)]


def make_weights(projector_type, seed, d_in=D_IN, d_out=D_OUT):
    """fp32 state dict under the reference's key names: matrices N(0, 1 / fan_in), biases N(0, 0.1^2), image_newline N(0, 1 / d_out)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for i, p in enumerate(linear_keys(projector_type)):
        k = d_in if i == 0 else d_out
        sd[p + "weight"] = torch.from_numpy((rs.standard_normal((d_out, k)) / math.sqrt(k)).astype(np.float32))
        sd[p + "bias"] = torch.from_numpy((0.1 * rs.standard_normal(d_out)).astype(np.float32))
    sd["image_newline"] = torch.from_numpy((rs.standard_normal(d_out) / math.sqrt(d_out)).astype(np.float32))
    return sd


def make_features(seed, frames, P, d_in=D_IN):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((frames, P * P, d_in)).astype(np.float32))


def project(sd, projector_type, x, bf16_operands=False):
    """x [..., d_in] in the dtype of the computation; sd already in that dtype."""
    for i, p in enumerate(linear_keys(projector_type)):
        if i:
            x = activation(x, "gelu")
        x = operand_linear(x, sd[p + "weight"], sd[p + "bias"], bf16_operands)
    return x


def pooled_side(P, mode, stride):
    if stride <= 1 or mode == "none":
        return P
    return -(-P // stride) if mode == "bilinear" else P // stride


def tap_matrix(P, mode, stride, dtype=torch.float64):
    """[P', P]: the 1-D taps of the average and bilinear pools (both are separable)."""
    Po = pooled_side(P, mode, stride)
    m = torch.zeros(Po, P, dtype=dtype)
    for o in range(Po):
        if mode == "average":
            m[o, o * stride:(o + 1) * stride] = 1.0 / stride
        elif mode == "bilinear":
            src = max((o + 0.5) * (P / Po) - 0.5, 0.0)
            i0 = min(int(math.floor(src)), P - 1)
            i1 = min(i0 + 1, P - 1)
            lam = src - i0
            m[o, i0] += 1.0 - lam
            m[o, i1] += lam
        else:
            m[o, o] = 1.0
    return m


def pool(x, P, mode, stride):
    """x [F, P * P, C] -> [F, P'^2, C] in x's dtype."""
    F, N, C = x.shape
    assert N == P * P
    if stride <= 1 or mode == "none":
        return x
    g = x.reshape(F, P, P, C)
    Po = pooled_side(P, mode, stride)
    if mode == "max":
        g = g[:, :Po * stride, :Po * stride].reshape(F, Po, stride, Po, stride, C)
        return g.amax(dim=(2, 4)).reshape(F, Po * Po, C)
    if mode not in ("average", "bilinear"):
        raise ValueError(f"Unexpected mm_spatial_pool_mode: {mode}")
    m = tap_matrix(P, mode, stride, x.dtype)
    return torch.einsum("oy,fyxc,px->fopc", m, g, m).reshape(F, Po * Po, C)


def effective_newline(cfg):
    merge = cfg.get("mm_patch_merge_type", "flat")
    pos = cfg.get("mm_newline_position", "one_token")
    if merge == "flat" or (pos == "one_token" and "unpad" not in merge):
        return "no_token"
    return pos


def add_newline(x, newline, position):
    """x [F, P'^2, C] -> [tokens, C]."""
    F, N, C = x.shape
    if position == "grid":
        Po = int(round(math.sqrt(N)))
        g = x.reshape(F, Po, Po, C)
        g = torch.cat([g, newline.to(x.dtype).expand(F, Po, 1, C)], dim=2)
        return g.reshape(F * Po * (Po + 1), C)
    if position == "frame":
        return torch.cat([x, newline.to(x.dtype).expand(F, 1, C)], dim=1).reshape(F * (N + 1), C)
    if position == "one_token":
        return torch.cat([x.reshape(F * N, C), newline.to(x.dtype)[None]], dim=0)
    if position == "no_token":
        return x.reshape(F * N, C)
    raise ValueError(f"Unexpected mm_newline_position: {position}")


def num_tokens(cfg, frames, P):
    Po = pooled_side(P, cfg.get("mm_spatial_pool_mode", "bilinear"), cfg.get("mm_spatial_pool_stride", 2))
    return {"grid": frames * Po * (Po + 1), "frame": frames * (Po * Po + 1), "one_token": frames * Po * Po + 1,
            "no_token": frames * Po * Po}[effective_newline(cfg)]


def forward(sd, cfg, feats, dtype=torch.float64, bf16_operands=False):
    """feats [F, P * P, d_in] -> [tokens, d_out] in ``dtype``: projector, then pool, then newline (the reference's order)."""
    W = {k: v.to(dtype) for k, v in sd.items()}
    x = feats.to(dtype)
    P = int(round(math.sqrt(x.shape[1])))
    y = project(W, cfg["mm_projector_type"], x, bf16_operands)
    y = pool(y, P, cfg.get("mm_spatial_pool_mode", "bilinear"), cfg.get("mm_spatial_pool_stride", 2))
    return add_newline(y, W.get("image_newline"), effective_newline(cfg))


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_weights(gold, projector_type):
    pre = f"w.{projector_type}."
    return {k[len(pre):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(pre) and k != pre + "seed"}


def golden_case(gold, name):
    """(state dict, config, features, the reference's fp32 output) of one F19 case."""
    proj = CASES[name][0]
    return golden_weights(gold, proj), case_config(name), torch.from_numpy(gold[f"{name}.features"]), torch.from_numpy(gold[f"{name}.output"])
