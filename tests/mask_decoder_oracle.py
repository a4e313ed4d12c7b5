"""Helper of the mask decoder tests (not a test file): the case table, the weight and input drawers and the whole forward of the reference's
``MultiScaleMaskedTransformerDecoder`` / ``CLMultiScaleMaskedTransformerDecoder`` (downstream/OVIS/mask2former/modeling/transformer_decoder/
mask2former_transformer_decoder.py, downstream/OVIS/ctvis/modeling/transformer_decoder/cl_mask2former_transformer_decoder.py) restated in
torch on the CPU, from the reference's operation order.  Nothing here imports the reference or the package under test.

    forward(sd, c, xs, mf, table="as_reference")      fp64 with the sine table computed in fp32 as PositionEmbeddingSine does even in a double
                                                      model: reproduces fixture F24 (tests/golden/f24_mask_decoder.npz, written by
                                                      tools/make_golden_mask_decoder.py)
    forward(sd, c, xs, mf, table="fp64")              everything in fp64: the ``want`` of the GPU tests
    forward(..., dtype=torch.float32, operands=m,     the same sequence in fp32 with the operands of every Linear rounded as the library's
            interp="features")                        compute mode does (m = "x3" / True) and the mask FEATURES resampled before the product
                                                      (the library's order; interpolation is linear): the PRECISION FLOOR of the GPU tests
    forward(..., masks=[m0, m1, ...])                 teacher forcing: layer i attends under masks[i] (bool [F, Q, hw] or packed int32)
                                                      instead of its own threshold

Every call returns the layers' own thresholds (``attn_masks``, after the reference's rule that clears a fully set row) and their
pre-threshold low-resolution logits (``low_logits``), whatever it attended under.

The draw makes the masks non-trivial: ``mask_embed.layers.2.bias`` is 0.5 + N(0, 0.1^2) and ``mask_features`` carry a per-pixel offset
that runs from -1 in the top rows to +1 in the bottom rows (frame 0) or stays negative (last frame), so logits are mostly far from zero
(few undecided bits), the top key tiles are hidden from whole query tiles, and the last frame's rows come out fully set and are cleared.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests.oracle_ops import layernorm, operand_linear
from tests.pixel_decoder_oracle import position_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f24_mask_decoder.npz")
LN_EPS = 1e-5
FRAMES = 2
LEVELS = 3

CASES = {
    # the base class; no input projection (in_channels == hidden_dim); head width 8; 100 queries = 6 full query tiles + 4; levels wrap
    "m2f": dict(cls="MultiScaleMaskedTransformerDecoder", in_channels=64, hidden=64, heads=8, queries=100, ffn=128, mask_dim=64, classes=7,
                layers=4, enforce=False, grids=[(2, 3), (4, 6), (7, 9)], mask_grid=(9, 11), seed=2401),
    # the CTVIS class; input projection because the widths differ; head width 32; fewer queries than a tile; one layer
    "cl": dict(cls="CLMultiScaleMaskedTransformerDecoder", in_channels=64, hidden=128, heads=4, queries=5, ffn=128, mask_dim=64, classes=3,
               layers=1, enforce=False, reid_hidden=64, reid_layers=3, grids=[(2, 3), (4, 6), (7, 9)], mask_grid=(8, 12), seed=2402),
    # the CTVIS class, projection enforced at equal widths, 100 queries, levels wrap
    "cl_wrap": dict(cls="CLMultiScaleMaskedTransformerDecoder", in_channels=64, hidden=64, heads=2, queries=100, ffn=64, mask_dim=64, classes=5,
                    layers=4, enforce=True, reid_hidden=64, reid_layers=2, grids=[(3, 2), (5, 7), (9, 7)], mask_grid=(6, 10), seed=2403),
}


def is_cl(c):
    return c["cls"].startswith("CL")


def decoder_kwargs(c):
    """Keyword arguments of the decoder class (the reference's and the library's) for a case, without ``in_channels``."""
    kw = dict(mask_classification=True, num_classes=c["classes"], hidden_dim=c["hidden"], num_queries=c["queries"], nheads=c["heads"],
              dim_feedforward=c["ffn"], dec_layers=c["layers"], pre_norm=False, mask_dim=c["mask_dim"], enforce_input_project=c["enforce"])
    if is_cl(c):
        kw.update(reid_hidden_dim=c["reid_hidden"], num_reid_head_layers=c["reid_layers"])
    return kw


def has_proj(c):
    return c["in_channels"] != c["hidden"] or c["enforce"]


def key_kinds(c):
    """name -> (kind, shape) in the reference's state-dict order."""
    C, ffn = c["hidden"], c["ffn"]
    k = OrderedDict()

    def affine(p):
        k[p + ".weight"], k[p + ".bias"] = ("scale", (C,)), ("bias", (C,))

    def lin(p, o, i, bias="bias"):
        k[p + ".weight"], k[p + ".bias"] = ("matrix", (o, i)), (bias, (o,))

    for group, attn in (("transformer_self_attention_layers", "self_attn"), ("transformer_cross_attention_layers", "multihead_attn")):
        for i in range(c["layers"]):
            p = f"{group}.{i}."
            k[p + attn + ".in_proj_weight"], k[p + attn + ".in_proj_bias"] = ("matrix", (3 * C, C)), ("bias", (3 * C,))
            lin(p + attn + ".out_proj", C, C)
            affine(p + "norm")
    for i in range(c["layers"]):
        p = f"transformer_ffn_layers.{i}."
        lin(p + "linear1", ffn, C)
        lin(p + "linear2", C, ffn)
        affine(p + "norm")
    affine("decoder_norm")
    k["query_feat.weight"] = ("embed", (c["queries"], C))
    k["query_embed.weight"] = ("embed", (c["queries"], C))
    k["level_embed.weight"] = ("embed", (LEVELS, C))
    if has_proj(c):
        for l in range(LEVELS):
            k[f"input_proj.{l}.weight"], k[f"input_proj.{l}.bias"] = ("matrix", (C, c["in_channels"], 1, 1)), ("bias", (C,))
    lin("class_embed", c["classes"] + 1, C)
    lin("mask_embed.layers.0", C, C)
    lin("mask_embed.layers.1", C, C)
    lin("mask_embed.layers.2", c["mask_dim"], C, bias="mask_bias")
    if is_cl(c):
        n, R = c["reid_layers"], c["reid_hidden"]
        dims = [C] + [R] * (n - 1) + [C]
        for j in range(n):
            lin(f"reid_embed.layers.{j}", dims[j + 1], dims[j])
    return k


def make_weights(c, seed=None):
    """The fp32 state dict of a case under the reference's names: matrices N(0, 1 / fan_in), biases N(0, 0.1^2), affine scales
    1 + N(0, 0.1^2), embeddings N(0, 1), the last mask_embed bias 0.5 + N(0, 0.1^2) (see the module docstring)."""
    rs = np.random.RandomState(c["seed"] if seed is None else seed)
    sd = OrderedDict()
    for k, (kind, shape) in key_kinds(c).items():
        z = rs.standard_normal(shape)
        v = {"matrix": lambda: z / np.sqrt(np.prod(shape[1:])), "bias": lambda: 0.1 * z, "scale": lambda: 1.0 + 0.1 * z, "embed": lambda: z,
             "mask_bias": lambda: 0.5 + 0.1 * z}[kind]()
        sd[k] = torch.from_numpy(np.asarray(v).astype(np.float32))
    return sd


def make_inputs(c, seed=None, frames=FRAMES):
    """([x0, x1, x2], mask_features): standard normal, mask_features plus the per-pixel offset of the module docstring; rounded to
    values fp16 holds exactly (the fixture stores the inputs as fp16)."""
    rs = np.random.RandomState((c["seed"] if seed is None else seed) + 7)
    fp16 = lambda a: torch.from_numpy(a.astype(np.float16).astype(np.float32))      # noqa: E731
    xs = [fp16(rs.standard_normal((frames, c["in_channels"], h, w))) for h, w in c["grids"]]
    H, W = c["mask_grid"]
    mf = rs.standard_normal((frames, c["mask_dim"], H, W))
    ramp = np.clip(3.0 * ((np.arange(H) + 0.5) / H - 0.5), -1.0, 1.0)[None, :, None]      # -1 in the top third, +1 in the bottom third
    offset = np.repeat(ramp, frames, 0)
    offset[-1] = -1.0                                                                     # the last frame: below zero everywhere
    return xs, fp16(mf + offset[:, None])


# ------------------------------------------------------------------------------------------------
# packed masks: bit (j & 31) of word j // 32 = key j, as the library stores them (int32 words)
# ------------------------------------------------------------------------------------------------
def pack_mask(m):
    m = np.asarray(m, dtype=bool)
    P = m.shape[-1]
    pad = (-P) % 32
    bits = np.concatenate([m, np.zeros(m.shape[:-1] + (pad,), bool)], -1)
    return np.packbits(bits, axis=-1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32).reshape(m.shape[:-1] + ((P + pad) // 32,))


def unpack_mask(words, P):
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32).astype("<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :P].astype(bool)


# ------------------------------------------------------------------------------------------------
# the pieces
# ------------------------------------------------------------------------------------------------
def attention(sd, p, q_in, k_in, v_in, heads, lin, mask=None):
    """nn.MultiheadAttention (unfused path: q scaled, additive -inf mask, softmax, out_proj) on [F, T, C] tensors; mask bool [F, Tq, Tk]."""
    W, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
    C = W.shape[1]
    hd = C // heads
    q, k, v = lin(q_in, W[:C], b[:C]), lin(k_in, W[C:2 * C], b[C:2 * C]), lin(v_in, W[2 * C:], b[2 * C:])
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, hd).transpose(1, 2)      # noqa: E731
    s = (split(q) * math.sqrt(1.0 / hd)) @ split(k).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask[:, None], float("-inf"))
    ctx = (torch.softmax(s, -1) @ split(v)).transpose(1, 2).reshape(q.shape)
    return lin(ctx, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def mlp(sd, p, x, n, lin):
    for j in range(n):
        x = lin(x, sd[f"{p}.layers.{j}.weight"], sd[f"{p}.layers.{j}.bias"])
        if j < n - 1:
            x = torch.relu(x)
    return x


def boxes_of(masks):
    """BitMasks(mask > 0).get_bounding_boxes() / (w, h, w, h), in fp32 as detectron2 computes it: [F, Q, 4]."""
    Fr, Q, H, W = masks.shape
    pos = masks > 0
    out = torch.zeros(Fr, Q, 4, dtype=torch.float32)
    xs, ys = pos.any(2), pos.any(3)
    for f in range(Fr):
        for q in range(Q):
            x, y = torch.where(xs[f, q])[0], torch.where(ys[f, q])[0]
            if len(x) > 0 and len(y) > 0:
                out[f, q] = torch.tensor([x[0], y[0], x[-1] + 1, y[-1] + 1], dtype=torch.float32)
    return out / torch.tensor([W, H, W, H], dtype=torch.float32)


def forward(sd, c, xs, mask_features, dtype=torch.float64, operands=False, table="fp64", masks=None, interp="logits"):
    """-> dict: pred_logits, pred_masks, (pred_queries, pred_embeds, pred_bboxes), aux (the reference's aux_outputs), attn_masks and
    low_logits per layer.  ``operands``: False, "x3" or True (tests/oracle_ops.py); ``interp``: "logits" (the reference's order) or
    "features" (the library's)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    xs = [x.to(dtype) for x in xs]
    mf = mask_features.to(dtype)
    lin = lambda x, w, b: operand_linear(x, w, b, operands)                    # noqa: E731
    C, heads, L, cl = c["hidden"], c["heads"], c["layers"], is_cl(c)
    Fr = mf.shape[0]
    src, pos, sizes = [], [], []
    for l, x in enumerate(xs):
        h, w = x.shape[2:]
        sizes.append((h, w))
        rows = x.flatten(2).transpose(1, 2)
        if has_proj(c):
            rows = lin(rows, sd[f"input_proj.{l}.weight"].reshape(C, -1), sd[f"input_proj.{l}.bias"])
        src.append(rows + sd["level_embed.weight"][l])
        pos.append(position_table(h, w, C, dtype, table).flatten(1).t()[None])
    qe = sd["query_embed.weight"][None].expand(Fr, -1, -1)
    out = sd["query_feat.weight"][None].expand(Fr, -1, -1)
    low_feats = {}

    def heads_of(out, size):
        dn = layernorm(out, sd["decoder_norm.weight"], sd["decoder_norm.bias"], LN_EPS)
        cls = lin(dn, sd["class_embed.weight"], sd["class_embed.bias"])
        me = mlp(sd, "mask_embed", dn, 3, lin)
        emb = (mlp(sd, "reid_embed", dn, c["reid_layers"], lin) if c["reid_layers"] > 0 else dn) if cl else None
        pm = torch.einsum("bqc,bchw->bqhw", me, mf)
        if interp == "features":
            if size not in low_feats:
                low_feats[size] = F.interpolate(mf, size=size, mode="bilinear", align_corners=False)
            low = torch.einsum("bqc,bchw->bqhw", me, low_feats[size])
        else:
            low = F.interpolate(pm, size=size, mode="bilinear", align_corners=False)
        return cls, pm, low.flatten(2), dn, emb

    preds = [heads_of(out, sizes[0])]
    own, lows = [], []
    for i in range(L):
        l = i % LEVELS
        low = preds[-1][2]
        m = low < 0
        m = m & ~m.all(-1, keepdim=True)                  # attn_mask[where(attn_mask.sum(-1) == HW)] = False
        own.append(m)
        lows.append(low)
        use = m
        if masks is not None:
            use = masks[i]
            if not torch.is_tensor(use) or use.dtype != torch.bool:
                use = torch.from_numpy(unpack_mask(use.cpu().numpy() if torch.is_tensor(use) else use, low.shape[-1]))
        p = f"transformer_cross_attention_layers.{i}."
        a = attention(sd, p + "multihead_attn.", out + qe, src[l] + pos[l], src[l], heads, lin, use)
        out = layernorm(out + a, sd[p + "norm.weight"], sd[p + "norm.bias"], LN_EPS)
        p = f"transformer_self_attention_layers.{i}."
        a = attention(sd, p + "self_attn.", out + qe, out + qe, out, heads, lin)
        out = layernorm(out + a, sd[p + "norm.weight"], sd[p + "norm.bias"], LN_EPS)
        p = f"transformer_ffn_layers.{i}."
        f2 = lin(torch.relu(lin(out, sd[p + "linear1.weight"], sd[p + "linear1.bias"])), sd[p + "linear2.weight"], sd[p + "linear2.bias"])
        out = layernorm(out + f2, sd[p + "norm.weight"], sd[p + "norm.bias"], LN_EPS)
        preds.append(heads_of(out, sizes[(i + 1) % LEVELS]))
    cls, pm, _, dn, emb = preds[-1]
    res = dict(pred_logits=cls, pred_masks=pm, attn_masks=own, low_logits=lows)
    if cl:
        res.update(pred_queries=dn, pred_embeds=emb, pred_bboxes=boxes_of(pm))
    res["aux"] = [dict(pred_logits=p[0], pred_masks=p[1], **(dict(pred_queries=p[3], pred_embeds=p[4]) if cl else {})) for p in preds[:-1]]
    return res


OUTPUTS = ("pred_logits", "pred_masks", "pred_queries", "pred_embeds", "pred_bboxes")


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
