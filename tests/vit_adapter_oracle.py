"""Helper of the ViT-Adapter tests (not a test file): the case table, the weight drawer and the whole forward of the reference's
``TimesformerMultiTaskingModelSigLIPViTAdapter`` (models/modeling_timesformer_siglip_adapter.py) restated in torch on the CPU, from the
reference's operation order.  Nothing here imports the reference; of the package only its seeded encoder weight drawer
(``init_weights.make_state_dict``) and its config class are used.

    forward(sd, case, pixels)                        fp64: reproduces fixture F22 (tests/golden/f22_vit_adapter.npz, written by
                                                     tools/make_golden_vit_adapter.py from the reference's own class in fp64)
    forward(..., dtype=torch.float32, operands=m)    the same sequence in fp32 with the operands of every Linear / GEMM rounded as the
                                                     library's compute mode does (m = "x3": bf16 hi + lo planes, three products; m = True:
                                                     one bf16 plane, and the attention operands q, k, v, p in bf16 too) and grid_sample as
                                                     the sampling operator: the PRECISION FLOOR of the GPU tests (tests/test_msda.py's rule)

The weights of a case are redrawn from its seed (numpy.random.RandomState for everything the adapter adds, make_state_dict for the
encoder); the fixture stores no weights.  Every tensor is drawn non-trivially, including what the reference's initialisation leaves at
zero or identity: sampling-offset weights, attention logits, biases, LayerNorm / BatchNorm affines, running_mean and a positive running_var.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import streamformer_oracle as O
from streamformer_amd.configuration import StreamformerConfig
from streamformer_amd.init_weights import make_state_dict
from tests import msda_oracle as MO
from tests.oracle_ops import bf16_round, operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f22_vit_adapter.npz")
INPLANES = 64            # the reference builds SpatialPriorModule(inplanes=64) whatever conv_inplane says (adapter:500)
BN_EPS = 1e-5
N_POINTS = 4

_SQ = dict(hidden=128, heads=2, layers=4, inter=256, indexes=[[0, 0], [1, 1], [2, 2], [3, 3]], deform_heads=2, cffn_ratio=0.5, image=64,
           frames=2, H=64, W=64, B=1, T=2, add_vit_feature=True, use_extra_extractor=True)
CASES = {
    "sq": dict(_SQ, seed=2201),
    # 64 x 96: patch grid 4 x 6, levels 8 x 12 / 4 x 6 / 2 x 3 — an H / W swap anywhere changes the result.  Two interaction blocks of two
    # layers each: the reference's forward unpacks exactly four kept ViT maps when add_vit_feature is set (adapter:661), so a model of two
    # blocks runs only without it; the ViT term on a non-square grid is covered at operator level (tests/test_vit_adapter.py, 4 x 6)
    "rect": dict(_SQ, indexes=[[0, 1], [2, 3]], H=64, W=96, B=2, T=1, add_vit_feature=False, seed=2202),
    "novit": dict(_SQ, add_vit_feature=False, use_extra_extractor=False, seed=2203),
}
OUTPUTS = ("res2", "res3", "res4", "res5")


def config(c):
    return StreamformerConfig(image_size=c["image"], patch_size=16, num_frames=c["frames"], hidden_size=c["hidden"],
                              num_hidden_layers=c["layers"], num_attention_heads=c["heads"], intermediate_size=c["inter"],
                              enable_causal_temporal=True)


def adapter_kwargs(c):
    """Constructor arguments of the adapter class (the reference's and the library's) for a case."""
    return dict(interaction_indexes=[list(p) for p in c["indexes"]], deform_num_heads=c["deform_heads"], cffn_ratio=c["cffn_ratio"],
                add_vit_feature=c["add_vit_feature"], use_extra_extractor=c["use_extra_extractor"], n_points=N_POINTS)


def grid(c):
    return c["H"] // 16, c["W"] // 16


def level_shapes(Hg, Wg):
    return [(2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2)]


def extractor_prefixes(c):
    last = len(c["indexes"]) - 1
    out = []
    for i in range(last + 1):
        block = [f"interactions.{i}.extractor."]
        if i == last and c["use_extra_extractor"]:
            block += [f"interactions.{i}.extra_extractors.{j}." for j in range(2)]
        out.append(block)
    return out


def adapter_key_kinds(c):
    """name -> (kind, shape) of everything the adapter adds to the encoder, in the reference's state-dict order."""
    D, hid = c["hidden"], int(c["hidden"] * c["cffn_ratio"])
    n_front = c["deform_heads"] * 1 * N_POINTS
    k = OrderedDict()

    def bn(p, ch):
        k[p + ".weight"], k[p + ".bias"] = ("scale", (ch,)), ("bias", (ch,))
        k[p + ".running_mean"], k[p + ".running_var"], k[p + ".num_batches_tracked"] = ("bias", (ch,)), ("var", (ch,)), ("count", ())

    def ln(p):
        k[p + ".weight"], k[p + ".bias"] = ("scale", (D,)), ("bias", (D,))

    def lin(p, o, i, kind="matrix"):
        k[p + ".weight"], k[p + ".bias"] = (kind, (o, i)), ("bias", (o,))

    k["level_embed"] = ("embed", (3, D))
    P = INPLANES
    for idx, (ci, co) in zip((0, 3, 6), ((3, P), (P, P), (P, P))):
        k[f"spm.stem.{idx}.weight"] = ("matrix", (co, ci, 3, 3))
        bn(f"spm.stem.{idx + 1}", co)
    for name, ci, co in (("conv2", P, 2 * P), ("conv3", 2 * P, 4 * P), ("conv4", 4 * P, 4 * P)):
        k[f"spm.{name}.0.weight"] = ("matrix", (co, ci, 3, 3))
        bn(f"spm.{name}.1", co)
    for name, ci in (("fc1", P), ("fc2", 2 * P), ("fc3", 4 * P), ("fc4", 4 * P)):
        k[f"spm.{name}.weight"], k[f"spm.{name}.bias"] = ("matrix", (D, ci, 1, 1)), ("bias", (D,))
    for block in extractor_prefixes(c):
        for p in block:
            ln(p + "query_norm")
            ln(p + "feat_norm")
            lin(p + "attn.sampling_offsets", 2 * n_front, D)
            k[p + "attn.sampling_offsets.bias"] = ("offset_bias", (2 * n_front,))
            lin(p + "attn.attention_weights", n_front, D)
            lin(p + "attn.value_proj", D, D)
            lin(p + "attn.output_proj", D, D)
            lin(p + "ffn.fc1", hid, D)
            k[p + "ffn.dwconv.dwconv.weight"], k[p + "ffn.dwconv.dwconv.bias"] = ("matrix", (hid, 1, 3, 3)), ("bias", (hid,))
            lin(p + "ffn.fc2", D, hid)
            ln(p + "ffn_norm")
    k["up.weight"], k["up.bias"] = ("matrix", (D, D, 2, 2)), ("bias", (D,))
    for i in range(1, 5):
        bn(f"norm{i}", D)
    return k


def make_weights(c, seed=None):
    """The fp32 state dict of a case under the reference's names, redrawn from its seed.  Matrices N(0, 1 / fan_in), biases and running
    means N(0, 0.1^2), affine scales 1 + N(0, 0.1^2), running_var uniform in [0.5, 1.5], the sampling-offset bias N(0, 1.5^2) so that the
    offsets spread over a few pixels, level_embed N(0, 1), num_batches_tracked 7."""
    seed = c["seed"] if seed is None else seed
    cfg = config(c)
    sd = OrderedDict((k, v) for k, v in make_state_dict(cfg, seed=seed).items() if not k.startswith("head."))
    for i in range(cfg.num_hidden_layers):
        sd[f"encoder.layer.{i}.temporal_attention.attention.mask"] = torch.tril(torch.ones(cfg.num_frames, cfg.num_frames))
    rs = np.random.RandomState(seed)
    for k, (kind, shape) in adapter_key_kinds(c).items():
        if kind == "count":
            sd[k] = torch.tensor(7, dtype=torch.int64)
            continue
        if kind == "var":
            v = rs.uniform(0.5, 1.5, shape)
        else:
            z = rs.standard_normal(shape)
            v = {"matrix": lambda: z / np.sqrt(np.prod(shape[1:])), "bias": lambda: 0.1 * z, "scale": lambda: 1.0 + 0.1 * z,
                 "offset_bias": lambda: 1.5 * z, "embed": lambda: z}[kind]()
        sd[k] = torch.from_numpy(np.asarray(v).astype(np.float32))
    return sd


def make_pixels(c, seed=None):
    """[B, T, 3, H, W] standard normal, rounded to values fp16 holds exactly (the fixture stores the input as fp16)."""
    rs = np.random.RandomState((c["seed"] if seed is None else seed) + 7)
    a = rs.standard_normal((c["B"], c["T"], 3, c["H"], c["W"]))
    return torch.from_numpy(a.astype(np.float16).astype(np.float32))


def reference_points(shapes):
    """get_reference_points (adapter:19-32): fp32 whatever the model's dtype is -> [1, sum H W, 1, 2] of (x, y)."""
    out = []
    for H_, W_ in shapes:
        ys = torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32) / H_
        xs = torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32) / W_
        ry, rx = torch.meshgrid(ys, xs, indexing="ij")
        out.append(torch.stack((rx.reshape(-1), ry.reshape(-1)), -1))
    return torch.cat(out, 0)[None, :, None, :]


# ------------------------------------------------------------------------------------------------
# the pieces
# ------------------------------------------------------------------------------------------------
def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)


def spatial_prior(sd, x):
    """SpatialPriorModule.forward (adapter:184-202): c1 NCHW at stride 4, c2..c4 as tokens at strides 8, 16, 32."""
    def block(x, conv, norm, stride):
        return F.relu(_bn(F.conv2d(x, sd[conv + ".weight"], None, stride, 1), sd, norm))
    c1 = block(x, "spm.stem.0", "spm.stem.1", 2)
    c1 = block(c1, "spm.stem.3", "spm.stem.4", 1)
    c1 = block(c1, "spm.stem.6", "spm.stem.7", 1)
    c1 = F.max_pool2d(c1, 3, 2, 1)
    c2 = block(c1, "spm.conv2.0", "spm.conv2.1", 2)
    c3 = block(c2, "spm.conv3.0", "spm.conv3.1", 2)
    c4 = block(c3, "spm.conv4.0", "spm.conv4.1", 2)
    fc = [F.conv2d(t, sd[f"spm.fc{i + 1}.weight"], sd[f"spm.fc{i + 1}.bias"]) for i, t in enumerate((c1, c2, c3, c4))]
    return (fc[0],) + tuple(t.flatten(2).transpose(1, 2) for t in fc[1:])


def dwconv(x, w, b, Hg, Wg):
    """DWConv.forward (adapter:244-254): one depthwise 3 x 3 on each of the three levels of [F, 21 n, C] on its own grid."""
    Fr, _, C = x.shape
    out, start = [], 0
    for H_, W_ in level_shapes(Hg, Wg):
        img = x[:, start:start + H_ * W_].transpose(1, 2).reshape(Fr, C, H_, W_)
        out.append(F.conv2d(img, w, b, 1, 1, groups=C).flatten(2).transpose(1, 2))
        start += H_ * W_
    return torch.cat(out, 1)


def encoder_layer(sd, cfg, i, h, lin, rnd):
    """TimesformerLayerSigLIP.forward (modeling:934-1004) frame-major, divided space-time, inference: oracle.layer_forward with the Linear
    (``lin(x, w, b)``) and the rounding of the attention operands (``rnd``) as arguments."""
    B, T, N, D = h.shape
    heads, eps, p = cfg.num_attention_heads, cfg.layer_norm_eps, f"encoder.layer.{i}."

    def L(x, name):
        return lin(x, sd[p + name + ".weight"], sd[p + name + ".bias"])

    def mha(q, k, v, mask):
        G, Lq, _ = q.shape
        d = D // heads
        qh, kh, vh = (rnd(t).reshape(G, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        s = (qh @ kh.transpose(-2, -1)) * (d ** -0.5)
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        return (rnd(s.softmax(-1)) @ vh).transpose(1, 2).reshape(G, Lq, D)

    q, k, v = L(O._ln(h, sd, p + "temporal_layernorm", eps), "temporal_attention.attention.qkv").split(D, -1)
    to_bn = lambda z: z.permute(0, 2, 1, 3).reshape(B * N, T, D)          # noqa: E731
    mask = (torch.arange(T)[None, :] <= torch.arange(T)[:, None]) if cfg.enable_causal_temporal else None
    ctx = mha(to_bn(q), to_bn(k), to_bn(v), mask).reshape(B, N, T, D).permute(0, 2, 1, 3)
    res_t = L(L(ctx, "temporal_attention.output.dense"), "temporal_dense")
    h1 = h + torch.tanh(sd[p + "temporal_attention_gating"]) * res_t
    q, k, v = L(O._ln(h1, sd, p + "layernorm_before", eps).reshape(B * T, N, D), "attention.attention.qkv").split(D, -1)
    h2 = h1 + L(mha(q, k, v, None), "attention.output.dense").reshape(B, T, N, D)
    return h2 + L(F.gelu(L(O._ln(h2, sd, p + "layernorm_after", eps), "intermediate.dense")), "output.dense")


def extractor(sd, p, c, query, feat, ref, Hg, Wg, eps, lin, operands, sample):
    """Extractor.forward (adapter:295-309): query + MSDeformAttn(LN(query), LN(feat)), then + ConvFFN(LN(.))."""
    ln = lambda x, name: F.layer_norm(x, (x.shape[-1],), sd[p + name + ".weight"], sd[p + name + ".bias"], eps)      # noqa: E731
    sub = {k[len(p) + 5:]: v for k, v in sd.items() if k.startswith(p + "attn.")}
    mc = dict(heads=c["deform_heads"], shapes=[(Hg, Wg)], P=N_POINTS)
    attn = MO.module(sub, mc, ln(query, "query_norm"), ln(feat, "feat_norm"), ref.expand(query.shape[0], -1, -1, -1), None, dtype=query.dtype,
                     bf16_operands=operands, sample=sample)
    query = query + attn
    y = lin(ln(query, "ffn_norm"), sd[p + "ffn.fc1.weight"], sd[p + "ffn.fc1.bias"])
    y = F.gelu(dwconv(y, sd[p + "ffn.dwconv.dwconv.weight"], sd[p + "ffn.dwconv.dwconv.bias"], Hg, Wg))
    return query + lin(y, sd[p + "ffn.fc2.weight"], sd[p + "ffn.fc2.bias"])


def tokens_to_map(t, H_, W_):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H_, W_)


def forward(sd, c, pixels, dtype=torch.float64, operands=False):
    """-> (OrderedDict res2..res5 NCHW, [c after every interaction block]).  ``operands``: False, "x3" or True (see the module docstring)."""
    cfg = config(c)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    px = pixels.to(dtype)
    lin = lambda x, w, b: operand_linear(x, w, b, operands)                    # noqa: E731
    rnd = bf16_round if operands is True else (lambda t: t)
    sample = MO.core_grid_sample if operands else MO.core
    B, T, _, H, W = px.shape
    Fr, D, (Hg, Wg) = B * T, cfg.hidden_size, (H // 16, W // 16)
    n = (Hg // 2) * (Wg // 2)
    c1, c2, c3, c4 = spatial_prior(sd, px.reshape(Fr, 3, H, W))
    le = sd["level_embed"]
    cc = torch.cat([c2 + le[0], c3 + le[1], c4 + le[2]], 1)
    w = sd["embeddings.patch_embeddings.projection.weight"]
    h = lin(O.patchify(px, 16), w.reshape(D, -1), sd["embeddings.patch_embeddings.projection.bias"])
    h = h + O.position_embedding(sd, cfg, H, W)[None, None] + O.time_embedding_rows(sd, cfg, 0, T, False)[None, :, None, :]
    ref = reference_points(level_shapes(Hg, Wg))
    outs, cs = [], []
    for (a, b), block in zip(c["indexes"], extractor_prefixes(c)):
        for i in range(a, b + 1):
            h = encoder_layer(sd, cfg, i, h, lin, rnd)
        feat = h.reshape(Fr, Hg * Wg, D)
        for p in block:
            cc = extractor(sd, p, c, cc, feat, ref, Hg, Wg, cfg.layer_norm_eps, lin, operands, sample)
        outs.append(tokens_to_map(feat, Hg, Wg))
        cs.append(cc)
    m2, m3, m4 = tokens_to_map(cc[:, :16 * n], 2 * Hg, 2 * Wg), tokens_to_map(cc[:, 16 * n:20 * n], Hg, Wg), tokens_to_map(cc[:, 20 * n:], Hg // 2, Wg // 2)
    if operands:        # the transposed convolution as the GEMM the library runs: rows = stride-8 pixels, columns (dy, dx, c_out)
        wl = sd["up.weight"].permute(2, 3, 1, 0).reshape(4 * D, D)
        up = lin(cc[:, :16 * n], wl, sd["up.bias"].repeat(4)).reshape(Fr, 2 * Hg, 2 * Wg, 2, 2, D)
        up = up.permute(0, 5, 1, 3, 2, 4).reshape(Fr, D, 4 * Hg, 4 * Wg)
    else:
        up = F.conv_transpose2d(m2, sd["up.weight"], sd["up.bias"], 2)
    m1 = up + c1
    if c["add_vit_feature"]:
        x1, x2, x3, x4 = outs
        m1 = m1 + F.interpolate(x1, scale_factor=4, mode="bilinear", align_corners=False)
        m2 = m2 + F.interpolate(x2, scale_factor=2, mode="bilinear", align_corners=False)
        m3 = m3 + x3
        m4 = m4 + F.interpolate(x4, scale_factor=0.5, mode="bilinear", align_corners=False)
    return OrderedDict((k, _bn(m, sd, f"norm{i + 1}")) for i, (k, m) in enumerate(zip(OUTPUTS, (m1, m2, m3, m4)))), cs


def golden_files(names):
    """path -> the array names it holds: the main file, and per case ``_<case>_res2`` and ``_<case>_c`` beside it (each part <= 1 MiB)."""
    stem = GOLDEN[:-len(".npz")]
    files = {GOLDEN: []}
    for k in names:
        case, leaf = k.split(".", 1)
        part = "res2" if leaf == "res2" else "c" if leaf[0] == "c" and leaf[1:].isdigit() else None
        files.setdefault(GOLDEN if part is None else f"{stem}_{case}_{part}.npz", []).append(k)
    return files


def load_golden():
    out = {}
    stem = GOLDEN[:-len(".npz")]
    for path in [GOLDEN] + [f"{stem}_{case}_{part}.npz" for case in CASES for part in ("res2", "c")]:
        with np.load(path, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out
