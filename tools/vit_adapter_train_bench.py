"""Training the ViT-Adapter on the MI355X: the two backward entries alone, and forward + backward of the whole adapter in training mode
under a frozen backbone, against torch on the same GPU.

    python tools/vit_adapter_train_bench.py            # -> profiles/vit_adapter_train.txt
    python tools/vit_adapter_train_bench.py --smoke    # one tiny shape, a few iterations, no file

(a) DWConv+GELU backward : sf_op_adapter_dwconv_gelu_backward (dx, dw, db; the workspace allocated outside the timed region) against the
                           autograd backward of the reference's operator sequence: three transposes to NCHW, three ``conv2d`` and a GELU.
                           F 16, 14 x 14 grid, C 192.  Achieved GB/s is over the bytes the backward must move: x and dy read, dx written.
    fuse adjoint         : sf_op_adapter_fuse_backward per level against the autograd backward of ``flatten(2).transpose(1, 2)`` made
                           contiguous (levels 1..3) and of the pixel shuffle (level 0).  F 16, 14 x 14 grid, D 768.
(b) adapter              : TimesformerMultiTaskingModelSigLIPViTAdapter(trainable=True).train(): forward, a scalar pairing with the four
                           outputs, backward to the adapter's parameters; against the same step of tools/vit_adapter_bench.py's torch
                           composition with the same weights.  1 and 8 clips of 16 x 224^2; ``torch.cuda.max_memory_allocated`` of one
                           step, measured from a reset peak.
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
from tools.pixel_decoder_train_bench import measure  # noqa: E402
from tools.vit_adapter_bench import composed_forward  # noqa: E402


def dwconv_entry(lines, Fr, C, H, W, warmup, iters, dev):
    tokens = 21 * (H // 2) * (W // 2)
    x, dy = torch.randn(Fr, tokens, C, device=dev), torch.randn(Fr, tokens, C, device=dev)
    w, b = torch.randn(C, 1, 3, 3, device=dev) / 3.0, 0.1 * torch.randn(C, device=dev)
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    ws = torch.empty(max(nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(Fr, H, W, C), 256), dtype=torch.uint8, device=dev)
    stream = nat.current_stream_handle(dev)

    def bwd():
        nat.check(nat.lib.sf_op_adapter_dwconv_gelu_backward(x.data_ptr(), w.data_ptr(), b.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                             db.data_ptr(), Fr, H, W, C, ws.data_ptr(), ws.numel(), stream))

    xt, wt, bt = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    parts, start = [], 0
    for H_, W_ in ((2 * H, 2 * W), (H, W), (H // 2, W // 2)):
        img = xt[:, start:start + H_ * W_].transpose(1, 2).reshape(Fr, C, H_, W_).contiguous()
        parts.append(F.conv2d(img, wt, bt, 1, 1, groups=C).flatten(2).transpose(1, 2))
        start += H_ * W_
    out = F.gelu(torch.cat(parts, 1))

    def t_bwd():
        xt.grad = wt.grad = bt.grad = None
        out.backward(dy, retain_graph=True)

    n_b, t_b = timed(bwd, warmup, iters)[0], timed(t_bwd, warmup, iters)[0]
    worst = max(float((g - t.grad).abs().max()) / float(t.grad.abs().max()) for g, t in ((dx, xt), (dw, wt), (db, bt)))
    gbytes = 12.0 * x.numel() / 1e9
    lines.append(f"(a) DWConv+GELU backward F={Fr} C={C} {H}x{W}: native {n_b:.3f} ({gbytes / n_b * 1e3:.0f} GB/s of the 12 bytes per element it must move), "
                 f"torch autograd {t_b:.3f} ({gbytes / t_b * 1e3:.0f} GB/s); workspace {ws.numel() / 2 ** 10:.0f} KiB; largest relative difference {worst:.1e}")
    print(lines[-1], flush=True)


def fuse_entry(lines, level, Fr, D, H, W, warmup, iters, dev):
    Ho, Wo = ((4 * H, 4 * W), (2 * H, 2 * W), (H, W), (H // 2, W // 2))[level]
    dy = torch.randn(Fr, D, Ho, Wo, device=dev)
    shape = (Fr, Ho * Wo // 4, 4 * D) if level == 0 else (Fr, Ho * Wo, D)
    d_tok = torch.empty(shape, device=dev)
    stream = nat.current_stream_handle(dev)

    def bwd():
        nat.check(nat.lib.sf_op_adapter_fuse_backward(level, dy.data_ptr(), d_tok.data_ptr(), shape[1] * shape[2], Fr, H, W, D, stream))

    tok = torch.randn(shape, device=dev).requires_grad_()
    if level == 0:
        out = tok.reshape(Fr, Ho // 2, Wo // 2, 2, 2, D).permute(0, 5, 1, 3, 2, 4).reshape(Fr, D, Ho, Wo)
    else:
        out = tok.transpose(1, 2).reshape(Fr, D, Ho, Wo).contiguous()

    def t_bwd():
        tok.grad = None
        out.backward(dy, retain_graph=True)

    n_b, t_b = timed(bwd, warmup, iters)[0], timed(t_bwd, warmup, iters)[0]
    same = torch.equal(d_tok, tok.grad)
    gbytes = 8.0 * dy.numel() / 1e9
    lines.append(f"(a) fuse adjoint level {level} F={Fr} D={D} {Ho}x{Wo}: native {n_b:.3f} ({gbytes / n_b * 1e3:.0f} GB/s of dy read + d_tokens written), "
                 f"torch autograd {t_b:.3f}; equal bits: {same}")
    print(lines[-1], flush=True)


def step(forward, module):
    """Forward, a pairing with the four outputs, backward to the adapter's parameters."""
    module.zero_grad(set_to_none=True)
    sum(t.square().mean() for t in forward().values()).backward()


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
        entry = dict(Fr=2, C=64, D=128, H=4, W=4)
    else:
        cfg, kw, shapes, size = sa.siglip_base(), {}, [(1, 16), (8, 16)], 224
        entry = dict(Fr=16, C=192, D=768, H=14, W=14)
    lines = [f"ViT-Adapter training step under a frozen backbone, hidden {cfg.hidden_size}, {cfg.num_hidden_layers} layers, {size} x {size}; fp32; median of "
             f"{args.iters} after {args.warmup} warm-up, HIP events; milliseconds, peak MiB of one step"]
    dwconv_entry(lines, entry["Fr"], entry["C"], entry["H"], entry["W"], args.warmup, args.iters, dev)
    for level in range(4):
        fuse_entry(lines, level, entry["Fr"], entry["D"], entry["H"], entry["W"], args.warmup, args.iters, dev)
    torch.manual_seed(0)
    m = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(cfg, trainable=True, **kw)
    for mod in m.modules():               # the reference's zero initialisation would make the sampling independent of the query
        if isinstance(mod, sa.MSDeformAttn):
            torch.nn.init.normal_(mod.sampling_offsets.weight, std=0.05)
            torch.nn.init.normal_(mod.attention_weights.weight, std=0.05)
    m = m.to(dev).train()
    m.embeddings.eval()                   # the composition calls the frozen encoder's sub-modules, which run in eval mode
    m.encoder.eval()
    for B, T in shapes:
        pixels = torch.randn(B, T, 3, size, size, device=dev)
        cells = []
        for what, fn in (("native", lambda: m(pixels)), ("torch", lambda: composed_forward(m, pixels))):
            ms, peak = measure(lambda: step(fn, m), args.warmup, args.iters)
            cells.append(f"{what} {ms:.2f} ms, peak {peak:.0f} MiB")
        a, b = m(pixels), composed_forward(m, pixels)
        worst = max(float((a[k] - b[k]).detach().abs().max()) / float(b[k].detach().abs().max()) for k in a)
        lines.append(f"(b) adapter forward + backward B={B} T={T}: " + "; ".join(cells) + f"; largest relative difference of the outputs {worst:.1e}")
        print(lines[-1], flush=True)
        del a, b
        torch.cuda.empty_cache()
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "vit_adapter_train.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
