"""ViT-Adapter forward on the MI355X: whole-forward time, its split, and the torch composition a user wrote before the module existed.

    python tools/vit_adapter_bench.py            # SigLIP-base, 224 x 224, 1 and 8 clips x 16 frames, both compute modes -> profiles/vit_adapter.txt
    python tools/vit_adapter_bench.py --smoke    # one tiny shape, a few iterations, no file (tests/test_vit_adapter.py)

native   : TimesformerMultiTaskingModelSigLIPViTAdapter.forward; the split comes from HIP events the module records between its stages
           (spatial prior module in torch, sf_embed, sf_layers, extractors, tail) in the same forwards.
composed : the same computation as a user of the library composed it in torch: the encoder's sub-module calls (patch-major in and out,
           so the stream is permuted around every block), torch LayerNorm / Linear / conv2d / interpolate / BatchNorm around
           ``ms_deform_attn``.  Same process, same weights, same input.
Timing: warm-up forwards, then HIP events around each forward, medians over the iterations.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
from tools._timing import timed  # noqa: E402


def composed_forward(m, pixel_values):
    """The reference's forward (adapter:596-680) in torch around the library's encoder sub-modules and ``ms_deform_attn``."""
    B, T, _, H, W = pixel_values.shape
    Fr, D, (Hg, Wg) = B * T, m.config.hidden_size, (H // 16, W // 16)
    n = (Hg // 2) * (Wg // 2)
    eps = m.config.layer_norm_eps
    ref, _ = m._geometry_for(Fr, Hg, Wg, pixel_values.device)
    c1, c2, c3, c4 = m.spm(pixel_values.reshape(Fr, 3, H, W))
    c = torch.cat([t.flatten(2).transpose(1, 2) + m.level_embed[i] for i, t in enumerate((c2, c3, c4))], 1)
    x = m.embeddings(pixel_values)                                           # (B, N * T, D), patch-major
    outs = []
    ln = lambda t, mod: F.layer_norm(t, (D,), mod.weight, mod.bias, eps)      # noqa: E731
    for block, (la, lb) in zip(m.interactions, m.interaction_indexes):
        for i in range(la, lb + 1):
            x = m.encoder.layer[i](x, T)[0]
        feat = x.reshape(B, -1, T, D).permute(0, 2, 1, 3).reshape(Fr, -1, D)
        for ex in block.extractors():
            a = ex.attn
            q, f = ln(c, ex.query_norm), ln(feat, ex.feat_norm)
            value = a.value_proj(f).view(Fr, -1, a.n_heads, D // a.n_heads)
            off = a.sampling_offsets(q).view(Fr, -1, a.n_heads, 1, a.n_points, 2)
            w = torch.softmax(a.attention_weights(q).view(Fr, -1, a.n_heads, a.n_points), -1).view(Fr, -1, a.n_heads, 1, a.n_points)
            loc = ref[:, :, None, :, None, :] + off / torch.tensor([Wg, Hg], device=q.device, dtype=q.dtype)
            c = c + a.output_proj(sa.ms_deform_attn(value, [(Hg, Wg)], None, loc, w))
            if ex.with_cffn:
                y = ex.ffn.fc1(ln(c, ex.ffn_norm))
                parts, start = [], 0
                for H_, W_ in ((2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2)):
                    img = y[:, start:start + H_ * W_].transpose(1, 2).reshape(Fr, -1, H_, W_).contiguous()
                    parts.append(ex.ffn.dwconv.dwconv(img).flatten(2).transpose(1, 2))
                    start += H_ * W_
                c = c + ex.ffn.fc2(F.gelu(torch.cat(parts, 1)))
        outs.append(feat.permute(0, 2, 1).reshape(Fr, D, Hg, Wg))
        x = feat.reshape(B, T, -1, D).permute(0, 2, 1, 3).reshape(B, -1, D)
    to_map = lambda t, h, w: t.transpose(1, 2).reshape(Fr, D, h, w).contiguous()      # noqa: E731
    m2, m3, m4 = to_map(c[:, :16 * n], 2 * Hg, 2 * Wg), to_map(c[:, 16 * n:20 * n], Hg, Wg), to_map(c[:, 20 * n:], Hg // 2, Wg // 2)
    m1 = m.up(m2) + c1
    if m.add_vit_feature:
        m1 = m1 + F.interpolate(outs[0], scale_factor=4, mode="bilinear", align_corners=False)
        m2 = m2 + F.interpolate(outs[1], scale_factor=2, mode="bilinear", align_corners=False)
        m3 = m3 + outs[2]
        m4 = m4 + F.interpolate(outs[3], scale_factor=0.5, mode="bilinear", align_corners=False)
    return {"res2": m.norm1(m1), "res3": m.norm2(m2), "res4": m.norm3(m3), "res5": m.norm4(m4)}


def split(m, pixels, iters):
    """Median milliseconds per stage over `iters` forwards, from the module's own event marks."""
    per = {}
    for _ in range(iters):
        m._marks = []
        m(pixels)
        torch.cuda.synchronize()
        marks, m._marks = m._marks, None
        run = {}
        for (_, e0), (stage, e1) in zip(marks, marks[1:]):
            run[stage] = run.get(stage, 0.0) + e0.elapsed_time(e1)
        for k, v in run.items():
            per.setdefault(k, []).append(v)
    return {k: statistics.median(v) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoke", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda:0")
    if args.smoke:
        cfg = sa.StreamformerConfig(image_size=64, num_frames=2, hidden_size=128, num_hidden_layers=4, num_attention_heads=2, intermediate_size=256,
                                    enable_causal_temporal=True)
        kw = dict(interaction_indexes=[[0, 0], [1, 1], [2, 2], [3, 3]], deform_num_heads=2, cffn_ratio=0.5)
        shapes, size, args.iters, args.warmup = [(1, 2)], 64, 2, 1
    else:
        cfg, kw, shapes, size = sa.siglip_base(), {}, [(1, 16), (8, 16)], 224
    lines = [f"ViT-Adapter forward, hidden {cfg.hidden_size}, {cfg.num_hidden_layers} layers, {size} x {size}; median of {args.iters} forwards after "
             f"{args.warmup} warm-up, HIP events; milliseconds"]
    torch.manual_seed(0)
    for mode in ("fp32", "bf16"):
        m = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(cfg, compute_dtype=mode, **kw).to(dev).eval()
        for B, T in shapes:
            pixels = torch.randn(B, T, 3, size, size, device=dev)
            with torch.no_grad():
                native = timed(lambda: m(pixels), warmup=args.warmup, iters=args.iters)[0]
                parts = split(m, pixels, args.iters)
                composed = timed(lambda: composed_forward(m, pixels), warmup=args.warmup, iters=args.iters)[0]
                a, b = m(pixels), composed_forward(m, pixels)
            worst = max(float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in a)
            lines.append(f"{mode} B={B} T={T}: native {native:.2f} (" + ", ".join(f"{k} {v:.2f}" for k, v in parts.items()) +
                         f"), composed {composed:.2f}, composed / native {composed / native:.2f}, largest relative difference {worst:.1e}")
            print(lines[-1], flush=True)
        del m
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "vit_adapter.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
