"""Time the spatial head's two new pieces at the benchmark batch (8 clips x 16 frames x 196 patches x 768, L = 100, masks 224 x 398):

  * ``sf_mask_loss`` forward + backward (one call): HIP events, median of --iters calls after --warmup;
  * the yardstick in the same process: the reference's operator sequence in torch on the GPU
    (normalize -> einsum -> interpolate -> cross_entropy, forward + backward, fp32), one clip at a time as the reference runs it,
    with its peak allocated bytes next to the fused call's;
  * the dense projection (``sf_dense_head_forward`` + ``sf_dense_head_backward``), beside the training micro-step it is added to.

    python tools/mask_loss_bench.py [--clips 8] [--iters 20] [--warmup 3] > profiles/r07_mask_loss.txt
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from streamformer_amd import _native as nat  # noqa: E402
from streamformer_amd.heads import DenseHeadProjection, MaskLossHead  # noqa: E402
from tools._timing import timed  # noqa: E402


def torch_sequence(x, tables, targets, ls, lb):
    """The reference's operators (modeling:1833-1836, 1885-1916), clip after clip, forward + backward."""
    x = x.detach().requires_grad_(True)
    ls = ls.detach().requires_grad_(True)
    lb = lb.detach().requires_grad_(True)
    losses = []
    P = int(round(x.shape[2] ** 0.5))
    for i in range(x.shape[0]):
        e = x[i] / x[i].norm(p=2, dim=-1, keepdim=True)
        z = torch.einsum("tpd,ld->tpl", e, tables[i]) * ls.exp() + lb
        z = z.reshape(z.shape[0], P, P, -1).permute(0, 3, 1, 2)
        z = F.interpolate(z, size=tuple(targets[i].shape[-2:]), mode="bilinear", align_corners=False)
        losses.append(F.cross_entropy(z, targets[i], ignore_index=-1))
    loss = torch.stack(losses).mean()
    loss.backward()
    return loss.detach(), x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, T, P, D, I, L, H, W = a.clips, 16, 14, 768, 3072, 100, 224, 398
    N = P * P
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, N, D, generator=g).to(dev)
    tables = []
    for _ in range(B):
        e = torch.randn(L, D, generator=g)
        tables.append((e / e.norm(dim=-1, keepdim=True)).to(dev))
    cells = torch.randint(-20, L, (B, T, 23, 23), generator=g).clamp_(min=-1)          # about a fifth of the cells ignored
    ys, xs = torch.arange(H) * 23 // H, torch.arange(W) * 23 // W
    targets = [cells[i][:, ys][:, :, xs].long().contiguous().to(dev) for i in range(B)]
    ls, lb = torch.log(torch.tensor(10.0)).to(dev), torch.tensor(-2.0).to(dev)
    print(f"# device: {torch.cuda.get_device_name(0)}; {B} clips x {T} frames x {N} patches x {D}, L = {L}, masks {H} x {W}; "
          f"median [min, max] of {a.iters} after {a.warmup} warm-up, HIP events")
    out = {}

    head = MaskLossHead(ls, lb)
    targets32 = [t.to(torch.int32) for t in targets]
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, gx, gs = head.loss(x, tables, targets32)
    torch.cuda.synchronize()
    fused_peak = torch.cuda.max_memory_allocated() - base
    med, lo, hi = timed(lambda: head.loss(x, tables, targets32), warmup=a.warmup, iters=a.iters)
    ws = nat.lib.sf_mask_loss_workspace_bytes(B, T, N, L)
    print(f"sf_mask_loss forward + backward      {med:8.3f} ms [{lo:.3f}, {hi:.3f}]   workspace {ws / 2**20:.1f} MiB, peak allocated above the inputs "
          f"{fused_peak / 2**20:.1f} MiB (workspace + d x)")
    out["mask_loss_ms"] = med
    out["mask_loss_workspace_bytes"] = int(ws)
    med1, lo1, hi1 = timed(lambda: head.loss(x, tables, targets32, need_grad=False), warmup=a.warmup, iters=a.iters)
    print(f"sf_mask_loss forward only            {med1:8.3f} ms [{lo1:.3f}, {hi1:.3f}]")
    out["mask_loss_forward_ms"] = med1

    if not a.skip_torch:
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tl, tgx = torch_sequence(x, tables, targets, ls, lb)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        medt, lot, hit = timed(lambda: torch_sequence(x, tables, targets, ls, lb), warmup=2, iters=max(5, a.iters // 2))
        err = float((gx - tgx).abs().max() / tgx.abs().max())
        print(f"torch operator sequence (fp32)       {medt:8.3f} ms [{lot:.3f}, {hit:.3f}]   peak allocated above the inputs {peak / 2**20:.1f} MiB "
              f"(upsampled logits of one clip: {T * L * H * W * 4 / 2**20:.0f} MiB)")
        print(f"  same loss: fused {float(loss):.6f}, torch {float(tl):.6f}; d x max-abs difference over max-abs {err:.2e}")
        out.update(torch_ms=medt, torch_peak_bytes=int(peak), speedup=medt / med)
        del tgx

    M = B * T * N
    g2 = torch.Generator().manual_seed(8)
    params = [torch.randn(D, D, generator=g2) * D ** -0.5, torch.zeros(D), torch.randn(D, D, generator=g2) * D ** -0.5, torch.zeros(D),
              torch.ones(D), torch.zeros(D), torch.randn(I, D, generator=g2) * D ** -0.5, torch.zeros(I),
              torch.randn(D, I, generator=g2) * I ** -0.5, torch.zeros(D)]
    params = [p.to(dev) for p in params]
    proj = DenseHeadProjection(1e-6)
    go = torch.randn(B, T, N, D, generator=g2).to(dev)

    def fb():
        proj.forward(x, params)
        proj.backward(go)
    medf, lof, hif = timed(lambda: proj.forward(x, params), warmup=a.warmup, iters=a.iters)
    medd, lod, hid = timed(fb, warmup=a.warmup, iters=a.iters)
    wsd = nat.lib.sf_dense_head_workspace_bytes(M, D, I)
    print(f"dense projection forward             {medf:8.3f} ms [{lof:.3f}, {hif:.3f}]   M = {M} rows")
    print(f"dense projection forward + backward  {medd:8.3f} ms [{lod:.3f}, {hid:.3f}]   workspace {wsd / 2**20:.0f} MiB")
    print("  (the training micro-step these are added to: 28.2-28.5 ms at the same batch, profiles/r06_bench_line.json)")
    out.update(dense_forward_ms=medf, dense_forward_backward_ms=medd, dense_workspace_bytes=int(wsd))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
