"""Each forward stage on its own, against a high-precision reference of the same operation on IDENTICAL inputs.

The whole-forward tests (test_hip_parity.py) bound a stage by whatever the noisiest part of the chain upstream of it carries; here
every stage gets the bound of its own arithmetic, so that a kernel that is wrong by a small multiple of its real error fails:

  * pooling head (``model.head``, stage 8 of sf_post_head): fp32 tokens [F, N, D] against ``O.pooling_head`` in fp64.  The head's
    arithmetic is bf16x3 / fp32 in BOTH compute modes, so both modes share one bound, and they must agree with each other to it.
  * embeddings (``model.embeddings``, sf_embed): the bf16 mode against operand-matched rounding (pixels and patch weights rounded to
    bf16 exactly where the patch kernel rounds them, fp64 accumulation), the accurate mode against plain fp64.
  * one encoder layer (``model.encoder.layer[0]``, sf_layers), accurate mode, against ``O.layer_forward`` in fp64.  (bf16-mode layers
    are bounded by operand rounding; the 4e-2 bounds of test_hip_parity.py already sit near it.)

Every bound is about twice the max-abs measured on an MI355X, which is written next to it.
"""
import numpy as np
import pytest
import torch

from oracle import streamformer_oracle as O
from streamformer_amd.configuration import StreamformerConfig
from streamformer_amd.init_weights import make_state_dict
from tests.helpers import frames, maxabs
from tests.oracle_ops import bf16_round

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(name, cfg, seed, mode):
    """One model per (width, mode) for the module; returns (model, fp32 state dict, fp64 state dict)."""
    key = (name, mode)
    if key not in _MODELS:
        import streamformer_amd as sa
        assert torch.cuda.is_available(), "these tests need the MI355X"
        sd = make_state_dict(cfg, seed=seed)
        m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
        m.load_state_dict(sd)
        _MODELS[key] = (m.to("cuda").eval(), sd, O.cast_state_dict(sd, torch.float64))
    return _MODELS[key]


def _cfg(**kw):
    base = dict(image_size=224, patch_size=16, num_frames=16, num_hidden_layers=1, enable_causal_temporal=True)
    base.update(kw)
    return StreamformerConfig(**base)


# ------------------------------------------------------------------------------------------------
# 1. pooling head
# ------------------------------------------------------------------------------------------------
# D / heads: the MFMA probe kernels (head_dim 64, D <= 1024; 192 = six k-steps over four waves) and the generic fp32 workgroup
HEAD_WIDTHS = {
    "d128": dict(hidden_size=128, num_attention_heads=2, intermediate_size=256),
    "d192": dict(hidden_size=192, num_attention_heads=3, intermediate_size=384),
    "d768": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072),
    "d1024": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096),
    "hd72": dict(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, patch_size=14),
    "hd32": dict(hidden_size=128, num_attention_heads=4, intermediate_size=256),
}


def pool_splits(F, N):
    """sf_pool_splits (sf_pool_head.hip): token splits of the probe kernel; the partial softmaxes are merged when S > 1."""
    S = 1
    while S < 8 and F * S < 256 and (N + 2 * S - 1) // (2 * S) >= 16:
        S *= 2
    return S


# (F, N, large-magnitude tokens).  F <= 4: the row-vector tail (sf_rowlin), F >= 5: the F-row GEMM tail.
HEAD_CASES = [(1, 196, False), (2, 9, False), (3, 36, False), (4, 729, False), (4, 81, True),
              (7, 9, False), (9, 36, False), (6, 81, False), (5, 256, False), (64, 196, False), (8, 196, True)]
# every split count meets both tails
assert {(pool_splits(F, N), F <= 4) for F, N, _ in HEAD_CASES} >= {(s, r) for s in (1, 2, 4, 8) for r in (True, False)}
# relative to the largest |output|, so that the large-magnitude inputs (outputs up to 44 instead of about 3) share the bound: the head's
# error grows with its output.  Measured 1.6e-5 (largest over every width, case and mode; 3.3e-5 max-abs on the ordinary inputs).
# Both modes run the same head arithmetic: measured bit-identical.
HEAD_REL = 4e-5


def _tokens(F, N, D, seed, big):
    x = frames(seed, (F, N, D))
    if big:             # a few tokens of large magnitude: large scores stress the max subtraction and the split-softmax merge
        x[:, 1] *= 12.0
        x[:, N // 2] *= -9.0
        x[:, N - 1] *= 7.0
    return x


@pytest.mark.parametrize("width", list(HEAD_WIDTHS))
def test_pooling_head_vs_fp64(width):
    cfg = _cfg(**HEAD_WIDTHS[width])
    D = cfg.hidden_size
    worst, seen = {}, set()
    for F, N, big in HEAD_CASES:
        x = _tokens(F, N, D, 1000 + F * N, big)
        outs = {}
        for mode in ("fp32", "bf16"):
            m, sd, sd64 = _model(width, cfg, 40, mode)
            outs[mode] = m.head(x.cuda()).cpu()
        want = O.pooling_head(sd64, cfg, x.double())
        scale = float(want.abs().max())
        for mode, got in outs.items():
            worst[(mode, F, N, big)] = maxabs(got, want) / scale
        worst[("bf16-vs-fp32", F, N, big)] = maxabs(outs["bf16"], outs["fp32"]) / scale
        seen.add((pool_splits(F, N), F <= 4))
    for k, d in sorted(worst.items(), key=lambda kv: -kv[1])[:6]:
        print(f"[head {width}] {k} S={pool_splits(k[1], k[2])} max-abs / max|ref| {d:.3e}")
    assert max(worst.values()) <= HEAD_REL, max(worst.items(), key=lambda kv: kv[1])
    assert len(seen) == 8


# ------------------------------------------------------------------------------------------------
# 2. embeddings
# ------------------------------------------------------------------------------------------------
EMB_CFGS = {
    "base": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072),
    "p14": dict(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, patch_size=14),
}
# (config, B, T, H, W, pixel dtype, clips compared).  B * T * N: one or two frames = the skinny GEMM, one or two clips = the tiles,
# eight clips = the 256^2 kernel.  T = 8 slices the 16-row time table, T = 32 repeats its rows (nearest).
EMB_CASES = [
    ("base", 1, 1, 224, 224, "f32", None), ("base", 2, 1, 224, 224, "u8", None), ("base", 1, 8, 224, 224, "bf16", None),
    ("base", 1, 16, 224, 224, "u8", None), ("base", 2, 16, 224, 224, "f32", None), ("base", 1, 32, 224, 224, "bf16", None),
    ("base", 8, 16, 224, 224, "u8", (0, 7)), ("base", 8, 16, 224, 224, "f32", (0, 7)),
    ("base", 1, 4, 160, 288, "f32", None), ("base", 2, 2, 224, 160, "u8", None),
    ("p14", 1, 2, 224, 224, "u8", None), ("p14", 2, 16, 224, 224, "f32", None), ("p14", 1, 3, 168, 252, "bf16", None),
]
# accurate mode against fp64: measured 2.6e-5 (fp32 pixels; 1.4e-5 for bf16 / uint8 pixels, whose lo plane is zero);
# bf16 mode against the operand-matched reference: measured 2.6e-6 (fp32 accumulation and output rounding)
EMB_TOL = {"fp32": 6e-5, "bf16": 6e-6}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", EMB_CASES, ids=lambda c: "-".join(str(v) for v in c[:6]))
def test_embeddings_vs_reference(mode, case):
    name, B, T, H, W, dt, clips = case
    cfg = _cfg(**EMB_CFGS[name])
    m, sd, sd64 = _model("emb-" + name, cfg, 50, mode)
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + H + W)
    if dt == "u8":
        x = torch.randint(0, 256, (B, T, 3, H, W), generator=g, dtype=torch.uint8)
        ip = m.image_processor           # sf_set_pixel_normalization: scale = rescale / std, shift = -mean / std in fp32,
        mean = np.float32(ip.image_mean[0])    # then one fp32 FMA per pixel (sf_patchify_kernel)
        std = np.float32(ip.image_std[0])
        assert all(v == ip.image_mean[0] for v in ip.image_mean) and all(v == ip.image_std[0] for v in ip.image_std)
        sc, sh = float(np.float32(ip.rescale_factor) / std), float(-mean / std)
        pix = (x.double() * sc + sh).float().double()     # u8 * fp32 scale is exact in fp64: one rounding to fp32 = fmaf
    else:
        xf = torch.randn(B, T, 3, H, W, generator=g)
        x = xf.to(torch.bfloat16) if dt == "bf16" else xf
        pix = x.double()
    got = m.embeddings(x.cuda()).cpu()
    Np = (H // cfg.patch_size) * (W // cfg.patch_size)
    got = got.reshape(B, Np, T, cfg.hidden_size).permute(0, 2, 1, 3)
    sel = list(clips) if clips else list(range(B))
    w = sd64["embeddings.patch_embeddings.projection.weight"]
    w = w.reshape(w.shape[0], -1)
    pat = O.patchify(pix[sel], cfg.patch_size)
    if mode == "bf16":          # the patch kernel rounds each pixel value (after the uint8 FMA) to bf16; the weights are bf16
        pat, w = bf16_round(pat), bf16_round(w)
    want = pat @ w.t() + sd64["embeddings.patch_embeddings.projection.bias"]
    want = want + O.position_embedding(sd, cfg, H, W).double()[None, None]        # bicubic table in fp32, as the model builds it
    want = want + O.time_embedding_rows(sd64, cfg, 0, T, False)[None, :, None, :]
    d = maxabs(got[sel], want)
    print(f"[embeddings {mode}] {case} max-abs {d:.3e}")
    assert d <= EMB_TOL[mode]


# ------------------------------------------------------------------------------------------------
# 3. one encoder layer, accurate mode
# ------------------------------------------------------------------------------------------------
LAYER_CFGS = {
    "base": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072),
    "base-noncausal": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, enable_causal_temporal=False),
    "d1024": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096),
    "hd72": dict(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, patch_size=14),        # 256 patches at 224^2
    "base384": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, image_size=384),     # 576 patches: streamed keys
}
# (config, B, T): one frame and four frames (small-M in-kernel LayerNorm fold), one clip, four clips
LAYER_CASES = [("base", 1, 1), ("base", 1, 4), ("base", 1, 16), ("base", 4, 16), ("base-noncausal", 1, 16),
               ("d1024", 1, 4), ("d1024", 1, 16), ("hd72", 1, 4), ("base384", 1, 4)]
LAYER_TOL = 7e-5          # measured 3.3e-5 (head_dim 72 / 14 x 14 layer; 2.2-2.7e-5 at head_dim 64, 3.2e-5 at N = 576)


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_encoder_layer_vs_fp64(case):
    name, B, T = case
    cfg = _cfg(**LAYER_CFGS[name])
    m, sd, sd64 = _model("layer-" + name, cfg, 60, "fp32")
    S = cfg.image_size
    h = O.embeddings(sd, cfg, frames(70 + B * T, (B, T, 3, S, S)))       # a realistic residual stream [B, T, N, D], fp32
    B_, T_, N, D = h.shape
    got = m.encoder.layer[0](O.to_patch_major(h).cuda(), T)[0].cpu()
    got = got.reshape(B, N, T, D).permute(0, 2, 1, 3)
    want = O.layer_forward(sd64, cfg, 0, h.double())
    d = maxabs(got, want)
    print(f"[layer fp32] {case} max-abs {d:.3e} (|h| max {float(want.abs().max()):.2f})")
    assert d <= LAYER_TOL
