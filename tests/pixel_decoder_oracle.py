"""Helper of the pixel decoder tests (not a test file): the case table, the weight drawer and the whole forward of the reference's
``MSDeformAttnPixelDecoder`` (downstream/OVIS/mask2former/modeling/pixel_decoder/msdeformattn.py) restated in torch on the CPU, from the
reference's operation order.  Nothing here imports the reference or the package under test.

    forward(sd, case, feats, table="as_reference")    fp64 with the position table and the reference points computed in fp32 as the
                                                      reference's classes do even in a double model: reproduces fixture F23
                                                      (tests/golden/f23_pixel_decoder.npz, written by tools/make_golden_pixel_decoder.py)
    forward(sd, case, feats, table="fp64")            everything in fp64: the ``want`` of the GPU tests (a floor taken against the fp32
                                                      table would be blind to the kernel's own table error)
    forward(..., dtype=torch.float32, operands=m)     the same sequence in fp32 with the operands of every GEMM rounded as the library's
                                                      compute mode does (m = "x3" / True) and grid_sample as the sampling operator: the
                                                      PRECISION FLOOR of the GPU tests

``make_weights`` redraws ALL weights from the case's seed, including what the reference initialises to zero (``sampling_offsets.weight``,
``attention_weights``: with those the sampling would not depend on the query); the fixture stores no weights.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests import msda_oracle as MO
from tests.oracle_ops import layernorm, operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f23_pixel_decoder.npz")
LEVELS = ("res2", "res3", "res4", "res5")
STRIDES = (4, 8, 16, 32)
N_POINTS = 4
GN_EPS = LN_EPS = 1e-5
FRAMES = 2

CASES = {
    # the shipped split: res3..res5 in the transformer, one FPN level; channels differ per level; grids that are no exact halves
    "m2f": dict(channels=(64, 128, 64, 192), grids=[(12, 20), (6, 10), (3, 5), (2, 3)], transformer=("res3", "res4", "res5"), conv_dim=64,
                heads=8, ffn=128, mask_dim=64, layers=2, seed=2301),
    # all four levels in the transformer: no FPN level, deformable attention over L = 4, GroupNorm over ONE pixel at the 1 x 1 level
    "all4": dict(channels=(64, 64, 128, 64), grids=[(8, 8), (4, 4), (2, 2), (1, 1)], transformer=LEVELS, conv_dim=128, heads=4, ffn=128,
                 mask_dim=64, layers=2, seed=2302),
    # one transformer level, three FPN levels chained: an FPN level upsamples an FPN output, at ratios 4 -> 7 and 7 -> 13
    "res5only": dict(channels=(64, 64, 128, 64), grids=[(13, 15), (7, 7), (4, 4), (2, 2)], transformer=("res5",), conv_dim=64, heads=8, ffn=64,
                     mask_dim=32, layers=2, seed=2303),
}


def decoder_kwargs(c):
    """Keyword arguments of the decoder class (the reference's and the library's) for a case, without ``input_shape``."""
    return dict(transformer_dropout=0.0, transformer_nheads=c["heads"], transformer_dim_feedforward=c["ffn"], transformer_enc_layers=c["layers"],
                conv_dim=c["conv_dim"], mask_dim=c["mask_dim"], norm="GN", transformer_in_features=list(c["transformer"]), common_stride=4)


def num_fpn(c):
    first = min(STRIDES[LEVELS.index(k)] for k in c["transformer"])
    return int(math.log2(first) - math.log2(4))


def transformer_levels(c):
    """Input level indices of the transformer's levels, coarsest first (the reference's order)."""
    return [i for i in range(3, -1, -1) if LEVELS[i] in c["transformer"]]


def out_levels(c):
    """Input level index of every entry of the reference's ``out`` list."""
    return transformer_levels(c) + list(range(num_fpn(c) - 1, -1, -1))


def key_kinds(c):
    """name -> (kind, shape) in the reference's state-dict order."""
    C, ffn, tr = c["conv_dim"], c["ffn"], transformer_levels(c)
    n = c["heads"] * len(tr) * N_POINTS
    k = OrderedDict()

    def affine(p):
        k[p + ".weight"], k[p + ".bias"] = ("scale", (C,)), ("bias", (C,))

    def lin(p, o, i):
        k[p + ".weight"], k[p + ".bias"] = ("matrix", (o, i)), ("bias", (o,))

    for j, l in enumerate(tr):
        k[f"input_proj.{j}.0.weight"], k[f"input_proj.{j}.0.bias"] = ("matrix", (C, c["channels"][l], 1, 1)), ("bias", (C,))
        affine(f"input_proj.{j}.1")
    k["transformer.level_embed"] = ("embed", (len(tr), C))
    for i in range(c["layers"]):
        p = f"transformer.encoder.layers.{i}."
        lin(p + "self_attn.sampling_offsets", 2 * n, C)
        k[p + "self_attn.sampling_offsets.bias"] = ("offset_bias", (2 * n,))
        lin(p + "self_attn.attention_weights", n, C)
        lin(p + "self_attn.value_proj", C, C)
        lin(p + "self_attn.output_proj", C, C)
        affine(p + "norm1")
        lin(p + "linear1", ffn, C)
        lin(p + "linear2", C, ffn)
        affine(p + "norm2")
    k["mask_features.weight"], k["mask_features.bias"] = ("matrix", (c["mask_dim"], C, 1, 1)), ("bias", (c["mask_dim"],))
    for idx in range(num_fpn(c)):
        k[f"adapter_{idx + 1}.weight"] = ("matrix", (C, c["channels"][idx], 1, 1))
        affine(f"adapter_{idx + 1}.norm")
        k[f"layer_{idx + 1}.weight"] = ("matrix", (C, C, 3, 3))
        affine(f"layer_{idx + 1}.norm")
    return k


def make_weights(c, seed=None):
    """The fp32 state dict of a case under the reference's names: matrices N(0, 1 / fan_in), biases N(0, 0.1^2), affine scales
    1 + N(0, 0.1^2), the sampling-offset bias N(0, 1.5^2) so that offsets spread over a few pixels, level_embed N(0, 1)."""
    rs = np.random.RandomState(c["seed"] if seed is None else seed)
    sd = OrderedDict()
    for k, (kind, shape) in key_kinds(c).items():
        z = rs.standard_normal(shape)
        v = {"matrix": lambda: z / np.sqrt(np.prod(shape[1:])), "bias": lambda: 0.1 * z, "scale": lambda: 1.0 + 0.1 * z,
             "offset_bias": lambda: 1.5 * z, "embed": lambda: z}[kind]()
        sd[k] = torch.from_numpy(np.asarray(v).astype(np.float32))
    return sd


def make_features(c, seed=None, frames=FRAMES):
    """name -> [F, C_l, H_l, W_l] standard normal, rounded to values fp16 holds exactly (the fixture stores the inputs as fp16)."""
    rs = np.random.RandomState((c["seed"] if seed is None else seed) + 7)
    return OrderedDict((k, torch.from_numpy(rs.standard_normal((frames, ch, H, W)).astype(np.float16).astype(np.float32)))
                       for k, ch, (H, W) in zip(LEVELS, c["channels"], c["grids"]))


# ------------------------------------------------------------------------------------------------
# the pieces
# ------------------------------------------------------------------------------------------------
def position_table(H, W, C, dtype=torch.float64, table="fp64"):
    """PositionEmbeddingSine(C / 2, normalize=True) of an all-false mask -> [C, H, W].  "as_reference": the class's own fp32 arithmetic
    (position_encoding.py:29-52), cast to ``dtype`` afterwards; "fp64": the formula in fp64."""
    wd = torch.float32 if table == "as_reference" else torch.float64
    npf = C // 2
    y = torch.arange(1, H + 1, dtype=wd)[:, None].expand(H, W)
    x = torch.arange(1, W + 1, dtype=wd)[None, :].expand(H, W)
    y = y / (y[-1:, :] + 1e-6) * (2 * math.pi)
    x = x / (x[:, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(npf, dtype=wd)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / npf)
    px, py = x[:, :, None] / dim_t, y[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).permute(2, 0, 1).to(dtype)


def reference_points(shapes, dtype=torch.float64, table="fp64"):
    """get_reference_points (msdeformattn.py:144-156) with valid ratios of 1 -> [1, S, L, 2] of (x, y)."""
    wd = torch.float32 if table == "as_reference" else torch.float64
    out = []
    for H, W in shapes:
        ys = torch.linspace(0.5, H - 0.5, H, dtype=wd) / H
        xs = torch.linspace(0.5, W - 0.5, W, dtype=wd) / W
        ry, rx = torch.meshgrid(ys, xs, indexing="ij")
        out.append(torch.stack((rx.reshape(-1), ry.reshape(-1)), -1))
    return torch.cat(out, 0)[None, :, None, :].expand(-1, -1, len(shapes), -1).to(dtype)


def to_rows(x):
    return x.flatten(2).transpose(1, 2)


def to_map(t, H, W):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H, W)


def conv1x1(x, w, b, lin):
    return to_map(lin(to_rows(x), w.reshape(w.shape[0], -1), b), x.shape[2], x.shape[3])


def conv3x3(x, w, lin):
    """padding 1, no bias, as a GEMM over the unfolded taps (the operand rounding of a compute mode is elementwise, so the tap order is free)."""
    cols = F.unfold(x, 3, padding=1).transpose(1, 2)                      # [F, H W, C * 9] in (c, dy, dx) order
    return to_map(lin(cols, w.reshape(w.shape[0], -1), None), x.shape[2], x.shape[3])


def group_norm(x, sd, p):
    return F.group_norm(x, 32, sd[p + ".weight"], sd[p + ".bias"], GN_EPS)


def forward(sd, c, feats, dtype=torch.float64, operands=False, table="fp64", locations=None):
    """-> (mask_features, [every entry of the reference's ``out``]).  ``operands``: False, "x3" or True (tests/oracle_ops.py); ``table``:
    "as_reference" or "fp64"; ``locations``: a list that receives the sampling locations of every encoder layer."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    feats = {k: v.to(dtype) for k, v in feats.items()}
    lin = lambda x, w, b: operand_linear(x, w, b, operands)                    # noqa: E731
    sample = MO.core_grid_sample if operands else MO.core
    C, tr = c["conv_dim"], transformer_levels(c)
    shapes = [c["grids"][l] for l in tr]
    srcs, poss = [], []
    for j, l in enumerate(tr):
        x = feats[LEVELS[l]]
        y = group_norm(conv1x1(x, sd[f"input_proj.{j}.0.weight"], sd[f"input_proj.{j}.0.bias"], lin), sd, f"input_proj.{j}.1")
        srcs.append(to_rows(y))
        poss.append(to_rows(position_table(*shapes[j], C, dtype, table)[None]) + sd["transformer.level_embed"][j])
    src, pos = torch.cat(srcs, 1), torch.cat(poss, 1)
    ref = reference_points(shapes, dtype, table).expand(src.shape[0], -1, -1, -1)
    mc = dict(heads=c["heads"], shapes=shapes, P=N_POINTS)
    for i in range(c["layers"]):
        p = f"transformer.encoder.layers.{i}."
        sub = {k[len(p) + 10:]: v for k, v in sd.items() if k.startswith(p + "self_attn.")}
        attn, _, _, _, loc, _ = MO.module(sub, mc, src + pos, src, ref, None, dtype=dtype, bf16_operands=operands, sample=sample, parts=True)
        if locations is not None:
            locations.append(loc)
        src = layernorm(src + attn, sd[p + "norm1.weight"], sd[p + "norm1.bias"], LN_EPS)
        ffn = lin(torch.relu(lin(src, sd[p + "linear1.weight"], sd[p + "linear1.bias"])), sd[p + "linear2.weight"], sd[p + "linear2.bias"])
        src = layernorm(src + ffn, sd[p + "norm2.weight"], sd[p + "norm2.bias"], LN_EPS)
    out, start = [], 0
    for H, W in shapes:
        out.append(to_map(src[:, start:start + H * W], H, W))
        start += H * W
    for k in range(num_fpn(c) - 1, -1, -1):
        x = feats[LEVELS[k]]
        cur = group_norm(conv1x1(x, sd[f"adapter_{k + 1}.weight"], None, lin), sd, f"adapter_{k + 1}.norm")
        y = cur + F.interpolate(out[-1], size=cur.shape[-2:], mode="bilinear", align_corners=False)
        out.append(torch.relu(group_norm(conv3x3(y, sd[f"layer_{k + 1}.weight"], lin), sd, f"layer_{k + 1}.norm")))
    return conv1x1(out[-1], sd["mask_features.weight"], sd["mask_features.bias"], lin), out


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
