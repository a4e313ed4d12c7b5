"""Training the Mask2Former pixel decoder on the MI355X: the two backward entries alone, and forward + backward of the whole decoder in
training mode, against torch on the same GPU.

    python tools/pixel_decoder_train_bench.py            # -> profiles/pixel_decoder_train.txt
    python tools/pixel_decoder_train_bench.py --smoke    # one tiny shape, a few iterations, no file

(a) GroupNorm backward : sf_op_pixdec_groupnorm_backward (dx, dgamma, dbeta; with ReLU; the workspace allocated outside the timed region)
                         against the autograd backward of ``relu(F.group_norm(x NCHW, 32))``; F 16, C 256, grids 56^2, 28^2, 14^2.  Achieved
                         GB/s is over the bytes the backward must move: x and dy read, dx written (12 bytes per element); the entry
                         itself reads x and dy twice (sums, then dx).
    upsample adjoint   : sf_op_pixdec_upsample_backward against the autograd backward of ``F.interpolate(bilinear)``, the FPN's shape
                         (28^2 -> 56^2, C 256, F 16).
(b) decoder            : MSDeformAttnPixelDecoder(trainable=True).train(): forward, a scalar pairing with the four outputs, backward to
                         the parameters and the inputs; against the same operator sequence in torch with the same weights
                         (tools/pixel_decoder_bench.py's composition: F.conv2d, F.group_norm, ms_deform_attn).  F = 2 and 16;
                         ``torch.cuda.max_memory_allocated`` of one step, measured from a reset peak.
Timing: warm-up steps, then HIP events around each step, medians (tools/_timing.py).  A cell where the native path loses is reported
as it is.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
import streamformer_amd._native as nat      # noqa: E402
from tools._timing import timed  # noqa: E402
from tools.pixel_decoder_bench import LEVELS, composed_forward  # noqa: E402


def measure(fn, warmup, iters):
    ms = timed(fn, warmup=warmup, iters=iters)[0]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return ms, torch.cuda.max_memory_allocated() / 2 ** 20


def groupnorm_entry(lines, Fr, C, H, W, warmup, iters, dev):
    x, dy = torch.randn(Fr, H * W, C, device=dev), torch.randn(Fr, H * W, C, device=dev)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
    stats, y = torch.empty(Fr, 32, 4, device=dev), torch.empty_like(x)
    dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    ws = torch.empty(max(nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(Fr, H, W, C), 256), dtype=torch.uint8, device=dev)
    stream = nat.current_stream_handle(dev)
    nat.check(nat.lib.sf_op_pixdec_groupnorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, None, 0, 0, None, stats.data_ptr(), y.data_ptr(), None, None,
                                             None, None, Fr, H, W, C, stream))

    def bwd():
        nat.check(nat.lib.sf_op_pixdec_groupnorm_backward(x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1, dy.data_ptr(), dx.data_ptr(),
                                                          dg.data_ptr(), db.data_ptr(), Fr, H, W, C, ws.data_ptr(), ws.numel(), stream))

    xt = x.transpose(1, 2).reshape(Fr, C, H, W).contiguous().requires_grad_()
    gt, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    dyt = dy.transpose(1, 2).reshape(Fr, C, H, W).contiguous()
    out = torch.relu(F.group_norm(xt, 32, gt, bt, 1e-5))

    def t_bwd():
        xt.grad = gt.grad = bt.grad = None
        out.backward(dyt, retain_graph=True)

    n_b, t_b = timed(bwd, warmup, iters)[0], timed(t_bwd, warmup, iters)[0]
    worst = max(float((dx.transpose(1, 2).reshape(Fr, C, H, W) - xt.grad).abs().max()), float((dg - gt.grad).abs().max()) / float(gt.grad.abs().max()),
                float((db - bt.grad).abs().max()) / float(bt.grad.abs().max()))
    gbytes = 12.0 * x.numel() / 1e9
    lines.append(f"(a) GroupNorm + ReLU backward F={Fr} C={C} {H}x{W}: native {n_b:.3f} ({gbytes / n_b * 1e3:.0f} GB/s of the 12 bytes per element it must move), "
                 f"torch autograd {t_b:.3f} ({gbytes / t_b * 1e3:.0f} GB/s); workspace {ws.numel() / 2 ** 10:.0f} KiB; largest difference {worst:.1e}")
    print(lines[-1], flush=True)


def upsample_entry(lines, Fr, C, Hp, Wp, H, W, warmup, iters, dev):
    dy, d_prev = torch.randn(Fr, H * W, C, device=dev), torch.empty(Fr, Hp * Wp, C, device=dev)
    stream = nat.current_stream_handle(dev)

    def bwd():
        nat.check(nat.lib.sf_op_pixdec_upsample_backward(dy.data_ptr(), d_prev.data_ptr(), Fr, H, W, Hp, Wp, C, stream))

    prev = torch.randn(Fr, C, Hp, Wp, device=dev).requires_grad_()
    dyt = dy.transpose(1, 2).reshape(Fr, C, H, W).contiguous()
    up = F.interpolate(prev, size=(H, W), mode="bilinear", align_corners=False)

    def t_bwd():
        prev.grad = None
        up.backward(dyt, retain_graph=True)

    n_b, t_b = timed(bwd, warmup, iters)[0], timed(t_bwd, warmup, iters)[0]
    worst = float((d_prev.transpose(1, 2).reshape(Fr, C, Hp, Wp) - prev.grad).abs().max())
    gbytes = 4.0 * (dy.numel() + d_prev.numel()) / 1e9
    lines.append(f"(a) upsample adjoint F={Fr} C={C} {Hp}x{Wp} <- {H}x{W}: native {n_b:.3f} ({gbytes / n_b * 1e3:.0f} GB/s of dy read + d_prev written), "
                 f"torch autograd {t_b:.3f}; largest difference {worst:.1e}")
    print(lines[-1], flush=True)


def step(forward, module, feats):
    """Forward, a pairing with the four outputs, backward to the parameters and the inputs."""
    module.zero_grad(set_to_none=True)
    for t in feats.values():
        t.grad = None
    mask, _, ms = forward()
    sum(t.square().mean() for t in [mask] + list(ms)).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoke", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[2, 16])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda:0")
    if args.smoke:
        cfg = dict(channels=128, conv_dim=64, heads=8, ffn=128, layers=2, mask_dim=64, grids=[(12, 20), (6, 10), (3, 5), (2, 3)])
        args.frames, args.iters, args.warmup = [2], 2, 1
        entry_f, entry_grids = 2, [(12, 20)]
    else:
        cfg = dict(channels=768, conv_dim=256, heads=8, ffn=1024, layers=6, mask_dim=256, grids=[(56, 56), (28, 28), (14, 14), (7, 7)])
        entry_f, entry_grids = 16, [(56, 56), (28, 28), (14, 14)]
    lines = [f"pixel decoder training step, conv_dim {cfg['conv_dim']}, {cfg['heads']} heads, ffn {cfg['ffn']}, {cfg['layers']} encoder layers, input "
             f"{cfg['channels']} channels, grids {cfg['grids']}; fp32; median of {args.iters} after {args.warmup} warm-up, HIP events; milliseconds, "
             "peak MiB of one step"]
    for H, W in entry_grids:
        groupnorm_entry(lines, entry_f, cfg["conv_dim"], H, W, args.warmup, args.iters, dev)
    (H, W), (Hp, Wp) = cfg["grids"][0], cfg["grids"][1]
    upsample_entry(lines, entry_f, cfg["conv_dim"], Hp, Wp, H, W, args.warmup, args.iters, dev)
    torch.manual_seed(0)
    m = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(cfg["channels"], s) for k, s in zip(LEVELS, (4, 8, 16, 32))}, transformer_dropout=0.0,
                                    transformer_nheads=cfg["heads"], transformer_dim_feedforward=cfg["ffn"], transformer_enc_layers=cfg["layers"],
                                    conv_dim=cfg["conv_dim"], mask_dim=cfg["mask_dim"], norm="GN", transformer_in_features=["res3", "res4", "res5"],
                                    common_stride=4, trainable=True)
    for mod in m.modules():               # the reference's zero initialisation would make the sampling independent of the query
        if isinstance(mod, sa.MSDeformAttn):
            torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.05)
            torch.nn.init.normal_(mod.attention_weights.weight, std=0.05)
    m = m.to(dev).train()
    for Fr in args.frames:
        feats = {k: torch.randn(Fr, cfg["channels"], H, W, device=dev).requires_grad_() for k, (H, W) in zip(LEVELS, cfg["grids"])}
        cells = []
        for what, fn in (("native", lambda: m.forward_features(feats)), ("torch", lambda: composed_forward(m, feats))):
            ms, peak = measure(lambda: step(fn, m, feats), args.warmup, args.iters)
            cells.append(f"{what} {ms:.2f} ms, peak {peak:.0f} MiB")
        a, b = m.forward_features(feats), composed_forward(m, feats)
        worst = max(float((x - y).detach().abs().max()) / float(y.detach().abs().max()) for x, y in zip([a[0]] + a[2], [b[0]] + b[2]))
        lines.append(f"(b) decoder forward + backward F={Fr}: " + "; ".join(cells) + f"; largest relative difference of the outputs {worst:.1e}")
        print(lines[-1], flush=True)
        del feats, a, b
        torch.cuda.empty_cache()
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "pixel_decoder_train.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
