"""Host cost per call of ``_native.launch`` against the written-out forms it replaced: N calls of sf_op_layernorm on 1 x 64 per loop in one
process, one synchronise at the end of each loop, the forms alternated over several rounds -> profiles/native_call.txt."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streamformer_amd import _native as nat  # noqa: E402

N, ROUNDS = 5000, 5
dev = torch.device("cuda", 0)
x, w, b = torch.randn(1, 64, device=dev), torch.ones(64, device=dev), torch.zeros(64, device=dev)
y = torch.empty_like(x)


def written_out():
    with torch.cuda.device(dev):
        nat.check(nat.lib.sf_op_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 1e-6, nat.current_stream_handle(dev)))


def written_out_unguarded():
    nat.check(nat.lib.sf_op_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 1e-6, nat.current_stream_handle(dev)))


def helper():
    nat.launch(dev, nat.lib.sf_op_layernorm, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 1e-6)


def helper_in_outer_guard():
    with torch.cuda.device(dev):
        nat.launch(dev, nat.lib.sf_op_layernorm, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 1e-6)


def written_out_two_guards():        # what launch cost inside a caller's guard before it skipped the entry for a current device
    with torch.cuda.device(dev):
        with torch.cuda.device(dev):
            nat.check(nat.lib.sf_op_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, 64, 1e-6, nat.current_stream_handle(dev)))


forms = (written_out, written_out_unguarded, written_out_two_guards, helper, helper_in_outer_guard)
for f in forms:
    for _ in range(200):
        f()
torch.cuda.synchronize()
res = {f.__name__: [] for f in forms}
for _ in range(ROUNDS):
    for f in forms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            f()
        torch.cuda.synchronize()
        res[f.__name__].append(1e6 * (time.perf_counter() - t0) / N)
print(f"per call, us: {N} calls of sf_op_layernorm 1 x 64 per loop, one synchronise at the end, {ROUNDS} rounds alternating the forms")
for k, v in res.items():
    print(f"  {k:24s} " + "  ".join(f"{t:6.2f}" for t in v) + f"   median {sorted(v)[len(v) // 2]:6.2f}")
