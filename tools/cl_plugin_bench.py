"""Forward + backward of the CTVIS contrastive loss without the matcher: the native ``CTCLPlugin`` on given indices against the oracle's
operator sequence (tests/cl_plugin_oracle.py ``reid_loss``) in torch fp32 on the same GPU.

    python tools/cl_plugin_bench.py [--out profiles/cl_plugin.txt]

Shape: the shipped one, 1 and 2 videos x 16 frames x 100 queries x 256 channels, 99 negatives, 8 instances of which 2 flicker.  Median of
10 after 3 warm-up runs; kernel launches by torch.profiler; host synchronisations of the torch side are its ``.item()``-style reads of
device tensors (``bool(tensor)`` of ``max(0, sim)`` and ``sim > 0``), counted by wrapping ``Tensor.__bool__``, ``item``, ``cpu`` and
``tolist``.  No threshold is asserted.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa                      # noqa: E402
from tests import cl_plugin_oracle as PO           # noqa: E402

F_, Q, C, NN, G = 16, 100, 256, 99, 8


def scenario(B, dev):
    rng = np.random.default_rng(5)
    valid = [[[not (i >= G - 2 and f % 3 == 1) for i in range(G)] for f in range(F_)] for _ in range(B)]
    g2q = [[[int(q) for q in rng.permutation(Q)[:G]] for _ in range(F_)] for _ in range(B)]
    e = torch.tensor(rng.standard_normal((B * F_, Q, C)).astype(np.float32) * 0.2, device=dev, requires_grad=True)
    indices = [[(torch.tensor(sorted(g2q[b][f])), torch.tensor(np.argsort(g2q[b][f]))) for b in range(B)] for f in range(F_)]
    targets = [[{"valid": torch.tensor(valid[b][f])} for b in range(B)] for f in range(F_)]
    return e, valid, PO.gt2query_of(indices, B), indices, targets


class Syncs:
    NAMES = ("__bool__", "item", "cpu", "tolist")

    def __enter__(self):
        self.n, self.real = 0, {k: getattr(torch.Tensor, k) for k in self.NAMES}
        for k, fn in self.real.items():
            def wrapped(t, *a, _fn=fn, **kw):
                self.n += bool(t.is_cuda)
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.real.items():
            setattr(torch.Tensor, k, fn)


def measure(step, e):
    def once():
        e.grad = None
        a, b = step()
        (2.0 * a + 3.0 * b).backward()
        torch.cuda.synchronize()
    for _ in range(3):
        once()
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        once()
        times.append((time.perf_counter() - t0) * 1e3)
    with Syncs() as s:
        once()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        once()
    launches = sum(ev.count for ev in prof.key_averages() if ev.device_type == torch.autograd.DeviceType.CUDA)
    return statistics.median(times), launches, s.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cl_plugin.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"CTVIS contrastive loss, forward + backward without the matcher: {F_} frames x {Q} queries x {C}, {NN} negatives, {G} instances (2 flicker)",
             "median of 10 (ms) | kernel launches | host synchronisations"]
    for B in (1, 2):
        e, valid, g2q, indices, targets = scenario(B, dev)
        coin = lambda: 0.75                        # noqa: E731  (both sides take the similarity-guided positive)
        plugin = sa.CTCLPlugin(weight_dict={}, num_negatives=NN, sampling_frame_num=F_, coin=coin)
        native = measure(lambda: tuple(plugin._reid(e, targets, indices).values()), e)
        torch_ = measure(lambda: PO.reid_loss(e, F_, NN, g2q, valid, True, None, coin)["losses"], e)
        items = plugin.plan(targets, indices, Q).I
        lines.append(f"B = {B} ({items} items): native {native[0]:.2f} ms | {native[1]} | {native[2]}    torch fp32 {torch_[0]:.2f} ms | {torch_[1]} | {torch_[2]}")
    text = "\n".join(lines)
    print(text)
    if not os.path.exists(args.out):
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
