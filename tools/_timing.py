"""Timing between HIP events, shared by the bench scripts of this directory (not a script).

    timed(fn, warmup, iters)      one event pair per call: (median, min, max) milliseconds
    compare(native, other, ...)   two callables in alternating windows of many calls each, so that clock and thermal drift
                                  hit both alike: ((median, min), (median, min)) milliseconds per call
"""
import statistics

import torch


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def compare(native, other, warmup, windows, target_ms, probe=3):
    """Alternating windows of the two callables; (median, min) milliseconds per call of each.  A window holds as many calls as
    fill ``target_ms``, sized from one window of ``probe`` calls, and never fewer than ``probe``."""
    for _ in range(warmup):
        native()
        other()
    torch.cuda.synchronize()
    calls = [max(probe, int(target_ms / max(window_ms(f, probe), 1e-3))) for f in (native, other)]
    a, b = [], []
    for _ in range(windows):
        a.append(window_ms(native, calls[0]))
        b.append(window_ms(other, calls[1]))
    return (statistics.median(a), min(a)), (statistics.median(b), min(b))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)
