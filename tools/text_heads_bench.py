"""Time the two kernels of the caption-driven heads at the benchmark batch (8 clips x 16 frames x 196 patches x 768, n = 8 captions):

  * ``sf_grounding_loss`` forward + backward (loss, d pooler, d scalars, logits) on pooler [8, 16, 768];
  * ``sf_dense_text_logits`` on the dense projection's 25 088 output rows, with the achieved GB/s against its algorithmic bytes
    (M D 4 in + M n 4 out);
  * next to each, the yardstick in the same process: the reference's operator sequence in torch on the same GPU, fp32
    (grounding: normalize -> einsum -> masked_fill -> logsigmoid, forward + backward; logits: normalize -> einsum -> scale + bias).

The library calls go straight through the C ABI on preallocated buffers (no allocation inside the timed region); HIP events around
every launch, median [min, max] of --iters launches after --warmup.

    python tools/text_heads_bench.py [--iters 30] [--warmup 5]
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
from tools._timing import timed  # noqa: E402


def torch_grounding(pooler, text, labels, ls, lb):
    p = pooler.detach().requires_grad_(True)
    s, b = ls.detach().requires_grad_(True), lb.detach().requires_grad_(True)
    img = p / p.norm(p=2, dim=-1, keepdim=True)
    txt = text / text.norm(p=2, dim=-1, keepdim=True)
    logits = torch.einsum("btd,bd->bt", img, txt) * s.exp() + b
    loss = -F.logsigmoid(labels.masked_fill(labels == 0, -1) * logits).sum() / logits.shape[0]
    loss.backward()
    return loss.detach(), p.grad, logits.detach()


def torch_logits(x, text, ls, lb):
    with torch.no_grad():
        xn = x / x.norm(p=2, dim=-1, keepdim=True)
        t = text / text.norm(p=2, dim=-1, keepdim=True)
        return torch.einsum("md,nd->mn", xn, t) * ls.exp() + lb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.iters >= 20
    dev = torch.device("cuda")
    B, T, N, D, n = 8, 16, 196, 768, 8
    M = B * T * N
    g = torch.Generator().manual_seed(9)
    pooler = torch.randn(B, T, D, generator=g).to(dev)
    text = torch.randn(n, D, generator=g).to(dev)
    labels = torch.randint(0, 2, (B, T), generator=g).float().to(dev)
    xs = [torch.randn(M, D, generator=g).to(dev) for _ in range(4)]      # 4 x 77 MB > the 256 MiB Infinity Cache: consecutive launches
    x, turn = xs[0], [0]                                                 # read different buffers, so every launch streams from HBM
    sc = torch.tensor([float(torch.log(torch.tensor(10.0))), -2.0], device=dev)
    ls, lb = sc[0:1], sc[1:2]
    stream = nat.current_stream_handle(dev)
    print(f"# device: {torch.cuda.get_device_name(0)}; {B} clips x {T} frames x {N} patches x {D}, n = {n} captions; "
          f"median [min, max] of {a.iters} launches after {a.warmup} warm-up, HIP events, device otherwise idle")
    out = {}

    loss, gp, gs, lg = torch.empty(1, device=dev), torch.empty_like(pooler), torch.empty(2, device=dev), torch.empty(B, T, device=dev)
    ws = torch.empty(nat.lib.sf_loss_workspace_bytes(B, T), dtype=torch.uint8, device=dev)

    def grounding():
        nat.check(nat.lib.sf_grounding_loss(pooler.data_ptr(), text.data_ptr(), labels.data_ptr(), B, T, D, ls.data_ptr(), lb.data_ptr(),
                                            loss.data_ptr(), gp.data_ptr(), gs.data_ptr(), lg.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    med, lo, hi = timed(grounding, warmup=a.warmup, iters=a.iters)
    medt, lot, hit = timed(lambda: torch_grounding(pooler, text, labels, ls[0], lb[0]), warmup=a.warmup, iters=a.iters)
    tl, tgp, tlg = torch_grounding(pooler, text, labels, ls[0], lb[0])
    torch.cuda.synchronize()
    print(f"sf_grounding_loss forward + backward   {med * 1e3:9.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}]   2 launches")
    print(f"torch operator sequence (fp32)         {medt * 1e3:9.1f} us [{lot * 1e3:.1f}, {hit * 1e3:.1f}]   forward + backward through autograd")
    print(f"  same loss: kernel {float(loss):.6f}, torch {float(tl):.6f}; d pooler max-abs difference over max-abs "
          f"{float((gp - tgp).abs().max() / tgp.abs().max()):.2e}; logits {float((lg - tlg).abs().max() / tlg.abs().max()):.2e}")
    out.update(grounding_us=med * 1e3, grounding_torch_us=medt * 1e3)

    o = torch.empty(M, n, device=dev)

    def nxt():
        turn[0] = (turn[0] + 1) % len(xs)
        return xs[turn[0]]

    def logits():
        nat.check(nat.lib.sf_dense_text_logits(nxt().data_ptr(), text.data_ptr(), M, D, n, ls.data_ptr(), lb.data_ptr(), o.data_ptr(), stream))
    med, lo, hi = timed(logits, warmup=a.warmup, iters=a.iters)
    medt, lot, hit = timed(lambda: torch_logits(nxt(), text, ls[0], lb[0]), warmup=a.warmup, iters=a.iters)
    turn[0] = len(xs) - 1
    logits()
    to = torch_logits(x, text, ls[0], lb[0])
    torch.cuda.synchronize()
    nbytes = M * D * 4 + M * n * 4
    print(f"sf_dense_text_logits                   {med * 1e3:9.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}]   {nbytes / 1e6:.1f} MB algorithmic "
          f"(M D 4 + M n 4) -> {nbytes / (med * 1e-3) / 1e9:.0f} GB/s")
    print(f"torch operator sequence (fp32)         {medt * 1e3:9.1f} us [{lot * 1e3:.1f}, {hit * 1e3:.1f}]   norm, divide, matmul, scale + bias")
    print(f"  same logits: max-abs difference over max-abs {float((o - to).abs().max() / to.abs().max()):.2e}")
    print("  (four input buffers in rotation, 308 MB > the 256 MiB Infinity Cache: every launch streams its rows from HBM)")
    out.update(dense_text_logits_us=med * 1e3, dense_text_logits_torch_us=medt * 1e3, dense_text_logits_gbps=nbytes / (med * 1e-3) / 1e9)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
