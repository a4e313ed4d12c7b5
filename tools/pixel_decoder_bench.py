"""Mask2Former pixel decoder forward on the MI355X against the torch composition a user wrote before the module existed.

    python tools/pixel_decoder_bench.py            # the shipped config (256 / 8 heads / 1024 / 6 layers, 768 input channels, grids 56, 28, 14, 7)
                                                   # at F = 16 and F = 128, both compute modes -> profiles/pixel_decoder.txt
    python tools/pixel_decoder_bench.py --smoke    # one tiny shape, a few iterations, no file

native   : MSDeformAttnPixelDecoder.forward_features (one sf_pixdec_forward call).  The whole forward is timed; a split by stage
           (projections, encoder layers, FPN, outputs) needs event marks inside the C forward and is not measured by this tool yet.
composed : the same operator sequence in torch on the same GPU, in the same process, with the same weights: F.conv2d, F.group_norm,
           the sine table and the reference points in torch, nn.Linear / LayerNorm around this repository's ``ms_deform_attn``.
Timing: warm-up forwards, then HIP events around each forward, medians over the iterations (tools/_timing.py).
"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
from tools._timing import timed  # noqa: E402

LEVELS = ("res2", "res3", "res4", "res5")


def sine_table(x, C):
    """PositionEmbeddingSine(C / 2, normalize=True) of an all-false mask for a map x [F, *, H, W] -> [1, C, H, W]."""
    H, W = x.shape[-2:]
    npf = C // 2
    y_embed = torch.arange(1, H + 1, dtype=torch.float32, device=x.device)[:, None].expand(H, W)
    x_embed = torch.arange(1, W + 1, dtype=torch.float32, device=x.device)[None, :].expand(H, W)
    y_embed = y_embed / (y_embed[-1:, :] + 1e-6) * (2 * math.pi)
    x_embed = x_embed / (x_embed[:, -1:] + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(npf, dtype=torch.float32, device=x.device)
    dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / npf)
    px, py = x_embed[:, :, None] / dim_t, y_embed[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).permute(2, 0, 1)[None]


def composed_forward(m, feats):
    """The reference's forward_features (msdeformattn.py:318-361) in torch around ``ms_deform_attn``."""
    C = m.conv_dim
    srcs, poss, shapes = [], [], []
    for idx, k in enumerate(m.transformer_in_features[::-1]):
        x = feats[k]
        srcs.append(m.input_proj[idx](x).flatten(2).transpose(1, 2))
        poss.append(sine_table(x, C).flatten(2).transpose(1, 2) + m.transformer.level_embed[idx])
        shapes.append(tuple(x.shape[-2:]))
    src, pos = torch.cat(srcs, 1), torch.cat(poss, 1)
    Fr, S, L = src.shape[0], src.shape[1], len(shapes)
    refs = []
    for H, W in shapes:
        ys = torch.linspace(0.5, H - 0.5, H, dtype=torch.float32, device=src.device) / H
        xs = torch.linspace(0.5, W - 0.5, W, dtype=torch.float32, device=src.device) / W
        ry, rx = torch.meshgrid(ys, xs, indexing="ij")
        refs.append(torch.stack((rx.reshape(-1), ry.reshape(-1)), -1))
    ref = torch.cat(refs, 0)[None, :, None, :]
    norm = torch.tensor([[W, H] for H, W in shapes], dtype=torch.float32, device=src.device)
    for layer in m.transformer.encoder.layers:
        a = layer.self_attn
        q = src + pos
        value = a.value_proj(src).view(Fr, S, a.n_heads, C // a.n_heads)
        off = a.sampling_offsets(q).view(Fr, S, a.n_heads, L, a.n_points, 2)
        w = torch.softmax(a.attention_weights(q).view(Fr, S, a.n_heads, L * a.n_points), -1).view(Fr, S, a.n_heads, L, a.n_points)
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        src = layer.norm1(src + a.output_proj(sa.ms_deform_attn(value, shapes, None, loc, w)))
        src = layer.norm2(src + layer.linear2(F.relu(layer.linear1(src))))
    out, start = [], 0
    for H, W in shapes:
        out.append(src[:, start:start + H * W].transpose(1, 2).reshape(Fr, C, H, W))
        start += H * W
    for k in range(m.num_fpn_levels - 1, -1, -1):
        lateral, output = getattr(m, f"adapter_{k + 1}"), getattr(m, f"layer_{k + 1}")
        cur = lateral.norm(F.conv2d(feats[m.in_features[k]], lateral.weight))
        y = cur + F.interpolate(out[-1], size=cur.shape[-2:], mode="bilinear", align_corners=False)
        out.append(F.relu(output.norm(F.conv2d(y, output.weight, None, 1, 1))))
    return F.conv2d(out[-1], m.mask_features.weight, m.mask_features.bias), out[0], out[:3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoke", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[16, 128])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda:0")
    if args.smoke:
        cfg = dict(channels=128, conv_dim=64, heads=8, ffn=128, layers=2, mask_dim=64, grids=[(12, 20), (6, 10), (3, 5), (2, 3)])
        args.frames, args.iters, args.warmup = [2], 2, 1
    else:
        cfg = dict(channels=768, conv_dim=256, heads=8, ffn=1024, layers=6, mask_dim=256, grids=[(56, 56), (28, 28), (14, 14), (7, 7)])
    lines = [f"pixel decoder forward, conv_dim {cfg['conv_dim']}, {cfg['heads']} heads, ffn {cfg['ffn']}, {cfg['layers']} encoder layers, input "
             f"{cfg['channels']} channels, grids {cfg['grids']}; median of {args.iters} forwards after {args.warmup} warm-up, HIP events; milliseconds"]
    for mode in ("fp32", "bf16"):
        torch.manual_seed(0)
        m = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(cfg["channels"], s) for k, s in zip(LEVELS, (4, 8, 16, 32))}, transformer_dropout=0.0,
                                        transformer_nheads=cfg["heads"], transformer_dim_feedforward=cfg["ffn"], transformer_enc_layers=cfg["layers"],
                                        conv_dim=cfg["conv_dim"], mask_dim=cfg["mask_dim"], norm="GN",
                                        transformer_in_features=["res3", "res4", "res5"], common_stride=4, compute_dtype=mode)
        for mod in m.modules():               # the reference's zero initialisation would make the sampling independent of the query
            if isinstance(mod, sa.MSDeformAttn):
                torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.05)
                torch.nn.init.normal_(mod.attention_weights.weight, std=0.05)
        m = m.to(dev).eval()
        for Fr in args.frames:
            feats = {k: torch.randn(Fr, cfg["channels"], H, W, device=dev) for k, (H, W) in zip(LEVELS, cfg["grids"])}
            with torch.no_grad():
                native = timed(lambda: m.forward_features(feats), warmup=args.warmup, iters=args.iters)[0]
                composed = timed(lambda: composed_forward(m, feats), warmup=args.warmup, iters=args.iters)[0]
                a, b = m.forward_features(feats), composed_forward(m, feats)
            worst = max(float((x - y).abs().max()) / float(y.abs().max()) for x, y in zip([a[0]] + a[2], [b[0]] + b[2]))
            lines.append(f"{mode} F={Fr}: native {native:.2f}, composed {composed:.2f}, composed / native {composed / native:.2f}, "
                         f"largest relative difference {worst:.1e}")
            print(lines[-1], flush=True)
            del feats, a, b
            torch.cuda.empty_cache()
        del m
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "pixel_decoder.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
