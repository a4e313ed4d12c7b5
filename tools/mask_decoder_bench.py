"""Mask2Former masked-attention decoder forward on the MI355X against the torch composition a user ran before the module existed.

    python tools/mask_decoder_bench.py            # the shipped config (256 / 8 heads / 2048 / 9 layers, Q = 100, mask_dim 256, 40 classes,
                                                  # 3 reid layers; 224^2 input: mask_features 56^2, levels 7^2, 14^2, 28^2) at F = 16 and
                                                  # F = 128, both compute modes, alone and behind the pixel decoder -> profiles/mask_decoder.txt
    python tools/mask_decoder_bench.py --smoke    # one tiny shape, a few iterations, no file

native   : CLMultiScaleMaskedTransformerDecoder.forward (one sf_maskdec_forward call); "chain": MSDeformAttnPixelDecoder.forward_features
           followed by it, the four tensors handed over as they are.
composed : the reference's operator sequence in torch on the same GPU, in the same process, with the same weights: the module's own
           ``nn.MultiheadAttention`` children with the boolean [B * heads, Q, HW] mask, ``F.interpolate`` of the [B, Q, H, W] logits,
           ``einsum``, nn.Linear / LayerNorm; "chain": the native pixel decoder followed by it (the torch pixel decoder is timed by
           tools/pixel_decoder_bench.py).
Timing: warm-up forwards, then HIP events around each forward, medians over the iterations (tools/_timing.py).  A cell where the native
path loses is reported as it is.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
from tools._timing import timed  # noqa: E402
from tools.pixel_decoder_bench import LEVELS, sine_table  # noqa: E402


def composed_forward(m, x, mask_features):
    """The reference's forward (cl_mask2former_transformer_decoder.py:177-272) in torch, [Q, B, C] order, without the aux list."""
    C, heads = m.hidden_dim, m.num_heads
    src, pos, sizes = [], [], []
    for i in range(3):
        sizes.append(x[i].shape[-2:])
        pos.append(sine_table(x[i], C).flatten(2).expand(x[i].shape[0], -1, -1).permute(2, 0, 1))
        p = m.input_proj[i]
        y = F.conv2d(x[i], p.weight, p.bias) if isinstance(p, sa.pixel_decoder.ConvNorm) else x[i]
        src.append((y.flatten(2) + m.level_embed.weight[i][None, :, None]).permute(2, 0, 1))
    bs = src[0].shape[1]
    qe = m.query_embed.weight.unsqueeze(1).repeat(1, bs, 1)
    out = m.query_feat.weight.unsqueeze(1).repeat(1, bs, 1)

    def heads_of(out, size):
        dn = m.decoder_norm(out).transpose(0, 1)
        cls = m.class_embed(dn)
        me = dn
        for j, layer in enumerate(m.mask_embed.layers):
            me = F.relu(layer(me)) if j < 2 else layer(me)
        emb = dn
        if isinstance(m.reid_embed, torch.nn.Identity):
            emb = dn
        else:
            n = len(m.reid_embed.layers)
            for j, layer in enumerate(m.reid_embed.layers):
                emb = F.relu(layer(emb)) if j < n - 1 else layer(emb)
        pm = torch.einsum("bqc,bchw->bqhw", me, mask_features)
        am = F.interpolate(pm, size=size, mode="bilinear", align_corners=False)
        am = (am.sigmoid().flatten(2).unsqueeze(1).repeat(1, heads, 1, 1).flatten(0, 1) < 0.5).bool()
        return cls, pm, am, dn, emb

    cls, pm, am, dn, emb = heads_of(out, sizes[0])
    for i in range(m.num_layers):
        l = i % 3
        am[torch.where(am.sum(-1) == am.shape[-1])] = False
        ca, sl, ff = m.transformer_cross_attention_layers[i], m.transformer_self_attention_layers[i], m.transformer_ffn_layers[i]
        out = ca.norm(out + ca.multihead_attn(query=out + qe, key=src[l] + pos[l], value=src[l], attn_mask=am)[0])
        out = sl.norm(out + sl.self_attn(out + qe, out + qe, value=out)[0])
        out = ff.norm(out + ff.linear2(F.relu(ff.linear1(out))))
        cls, pm, am, dn, emb = heads_of(out, sizes[(i + 1) % 3])
    return dict(pred_logits=cls, pred_masks=pm, pred_queries=dn, pred_embeds=emb)


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
        cfg = dict(channels=64, hidden=64, heads=8, ffn=128, layers=4, queries=20, mask_dim=64, classes=5, reid=2, pix_ffn=128, pix_layers=2,
                   grids=[(12, 20), (6, 10), (3, 5), (2, 3)])
        args.frames, args.iters, args.warmup = [2], 2, 1
    else:
        cfg = dict(channels=768, hidden=256, heads=8, ffn=2048, layers=9, queries=100, mask_dim=256, classes=40, reid=3, pix_ffn=1024, pix_layers=6,
                   grids=[(56, 56), (28, 28), (14, 14), (7, 7)])
    lines = [f"mask decoder forward, hidden {cfg['hidden']}, {cfg['heads']} heads, ffn {cfg['ffn']}, {cfg['layers']} layers, {cfg['queries']} queries, "
             f"mask_dim {cfg['mask_dim']}, {cfg['classes']} classes, {cfg['reid']} reid layers, grids {cfg['grids']}; median of {args.iters} forwards "
             f"after {args.warmup} warm-up, HIP events; milliseconds"]
    for mode in ("fp32", "bf16"):
        torch.manual_seed(0)
        pix = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(cfg["channels"], s) for k, s in zip(LEVELS, (4, 8, 16, 32))}, transformer_dropout=0.0,
                                          transformer_nheads=cfg["heads"], transformer_dim_feedforward=cfg["pix_ffn"],
                                          transformer_enc_layers=cfg["pix_layers"], conv_dim=cfg["hidden"], mask_dim=cfg["mask_dim"], norm="GN",
                                          transformer_in_features=["res3", "res4", "res5"], common_stride=4, compute_dtype=mode)
        for mod in pix.modules():
            if isinstance(mod, sa.MSDeformAttn):
                torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.05)
                torch.nn.init.normal_(mod.attention_weights.weight, std=0.05)
        pix = pix.to(dev).eval()
        m = sa.CLMultiScaleMaskedTransformerDecoder(cfg["hidden"], num_classes=cfg["classes"], hidden_dim=cfg["hidden"], num_queries=cfg["queries"],
                                                    nheads=cfg["heads"], dim_feedforward=cfg["ffn"], dec_layers=cfg["layers"], pre_norm=False,
                                                    mask_dim=cfg["mask_dim"], enforce_input_project=False, reid_hidden_dim=cfg["hidden"],
                                                    num_reid_head_layers=cfg["reid"], compute_dtype=mode).to(dev).eval()
        for Fr in args.frames:
            feats = {k: torch.randn(Fr, cfg["channels"], H, W, device=dev) for k, (H, W) in zip(LEVELS, cfg["grids"])}
            with torch.no_grad():
                mf, _, ms = pix.forward_features(feats)
                native = timed(lambda: m(ms, mf), warmup=args.warmup, iters=args.iters)[0]
                composed = timed(lambda: composed_forward(m, ms, mf), warmup=args.warmup, iters=args.iters)[0]
                def native_chain():
                    a, _, b = pix.forward_features(feats)
                    return m(b, a)

                chain = timed(native_chain, warmup=args.warmup, iters=args.iters)[0]

                def composed_chain():
                    a, _, b = pix.forward_features(feats)
                    return composed_forward(m, b, a)

                chain_c = timed(composed_chain, warmup=args.warmup, iters=args.iters)[0]
                a, b = m(ms, mf), composed_forward(m, ms, mf)
            worst = max(float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in b)
            lines.append(f"{mode} F={Fr}: native {native:.2f}, composed {composed:.2f}, composed / native {composed / native:.2f}; behind the pixel "
                         f"decoder: native {chain:.2f}, composed {chain_c:.2f}, composed / native {chain_c / chain:.2f}; largest relative "
                         f"difference {worst:.1e} (free-running: a flipped mask bit is not an error)")
            print(lines[-1], flush=True)
            del feats, a, b, mf, ms
            torch.cuda.empty_cache()
        del m, pix
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "mask_decoder.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
