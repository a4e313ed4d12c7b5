"""Forward + backward of MaskedMultiheadAttention against nn.MultiheadAttention under the boolean [F * heads, Q, HW] mask, same GPU,
same process, same weights.  Writes profiles/masked_attention.txt.

    python tools/masked_attention_bench.py [--out profiles/masked_attention.txt]

C 256, 8 heads, Q 100, F 16, HW in {49, 196, 784, 3600}, about 10 % and 90 % of the mask hidden (no fully hidden row).  HIP events,
median of 10 after 3 warm-up.  The native side is timed twice: from the boolean mask torch gets (packing included) and from a
PackedAttentionMask made once (what a decoder that keeps its masks packed pays).  Peak memory is torch.cuda.max_memory_allocated over one
forward + backward, above what is allocated before it.
"""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streamformer_amd import MaskedMultiheadAttention, pack_attention_mask      # noqa: E402

C, HEADS, Q, F = 256, 8, 100, 16


def _step(mod, x, y, mask, g):
    for t in (x, y, *mod.parameters()):
        t.grad = None
    out = mod(x, y, y, attn_mask=mask, need_weights=False)[0]
    out.backward(g)


def _time(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "masked_attention.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ref = nn.MultiheadAttention(C, HEADS).to(dev)
    nat = MaskedMultiheadAttention.from_torch(ref)
    lines = [f"masked attention, forward + backward: C {C}, {HEADS} heads, Q {Q}, F {F}; {torch.cuda.get_device_name(0)}",
             "median ms of 10 after 3 warm-up (HIP events); peak = max_memory_allocated over one step above the resident tensors, MiB",
             "torch = nn.MultiheadAttention with the bool [F * heads, Q, HW] mask; native = MaskedMultiheadAttention with the same mask "
             "(packing included); packed = with a PackedAttentionMask made once",
             f"{'HW':>5} {'hidden':>7} | {'torch ms':>9} {'native ms':>10} {'packed ms':>10} {'torch/native':>13} {'torch/packed':>13} | "
             f"{'torch MiB':>10} {'native MiB':>11} {'packed MiB':>11}"]
    for HW in (49, 196, 784, 3600):
        for hidden in (0.1, 0.9):
            x = torch.randn(Q, F, C, device=dev, requires_grad=True)
            y = torch.randn(HW, F, C, device=dev, requires_grad=True)
            g = torch.randn(Q, F, C, device=dev)
            mask = torch.rand(F, 1, Q, HW, device=dev) < hidden      # the reference's mask: one per frame, repeated over the heads
            mask[..., 0] = False
            mask = mask.expand(F, HEADS, Q, HW).reshape(F * HEADS, Q, HW).contiguous()
            packed = pack_attention_mask(mask[::HEADS].contiguous())
            runs = {"torch": lambda: _step(ref, x, y, mask, g), "native": lambda: _step(nat, x, y, mask, g),
                    "packed": lambda: _step(nat, x, y, packed, g)}
            ms = {k: _time(fn) for k, fn in runs.items()}
            mib = {k: _peak(fn) for k, fn in runs.items()}
            lines.append(f"{HW:>5} {hidden:>7.0%} | {ms['torch']:>9.3f} {ms['native']:>10.3f} {ms['packed']:>10.3f} "
                         f"{ms['torch'] / ms['native']:>13.2f} {ms['torch'] / ms['packed']:>13.2f} | "
                         f"{mib['torch']:>10.1f} {mib['native']:>11.1f} {mib['packed']:>11.1f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
