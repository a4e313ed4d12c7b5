"""Streaming step of 8 streams in one batched 64-frame cache (SigLIP-base, one new 224^2 frame per stream and call), p50 per call:

  one   one stream, one frame per call (bench.py's streaming.p50_ms quantity)
  (a)   the lockstep call: all 8 streams at the same position
  (b)   the ragged call (stream_ids): the 8 streams staggered 8 frames apart (stream i prefilled with 8 i frames, then 8 calls
        of all eight until the deepest one is full)
  (c)   eight private single-stream caches, one call each: what (b)'s workload costs without independent positions

Each quantity is measured REPS times (default 3) so that the spread of (a) is there to judge (b) - (a) against; the first pass of
every measurement is warm-up.  On a checkout without stream_ids, `one`, (a) and (c) still run.  SF_MODES=bf16,fp32  SF_REPS=3"""
import inspect, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, streamformer_amd as sa

S, CAP, STEP = 8, 64, 8
REPS = int(os.environ.get("SF_REPS", "3"))
cfg = sa.siglip_base(num_frames=CAP)
HAS_RAGGED = "stream_ids" in inspect.signature(sa.TimesformerMultiTaskingModelSigLIP.forward).parameters


def p50(v):
    v = sorted(v)
    return v[len(v) // 2] * 1e3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def lockstep(m, x, streams, passes=3):
    cache = m.new_cache(streams, CAP)
    lat = []
    for rep in range(passes):
        cache.reset()
        for t in range(CAP):
            dt = timed(lambda: m(x[:streams, t:t + 1], use_cache=True, past_key_values=cache))
            if rep:
                lat.append(dt)
    return p50(lat)


def ragged(m, x, passes=7):
    cache = m.new_cache(S, CAP)
    ids = list(range(S))
    # row i of call k is frame 8 i + k of stream i; the call takes a strided slice, like the lockstep call does
    xb = torch.stack([x[i, STEP * i:STEP * i + STEP] for i in ids])
    lat = []
    for rep in range(passes):
        cache.reset()
        for i in range(1, S):
            m(x[i:i + 1, :STEP * i], past_key_values=cache, stream_ids=[i])
        for k in range(STEP):
            dt = timed(lambda: m(xb[:, k:k + 1], past_key_values=cache, stream_ids=ids))
            if rep:
                lat.append(dt)
    return p50(lat)


def private(m, x, passes=3):
    caches = [m.new_cache(1, CAP) for _ in range(S)]
    lat = []
    for rep in range(passes):
        for c in caches:
            c.reset()
        for t in range(CAP):
            def step():
                for i, c in enumerate(caches):
                    m(x[i:i + 1, t:t + 1], use_cache=True, past_key_values=c)
            dt = timed(step)
            if rep:
                lat.append(dt)
    return p50(lat)


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; stream_ids available: {HAS_RAGGED}")
    for mode in os.environ.get("SF_MODES", "bf16,fp32").split(","):
        m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
        m.load_state_dict(sa.make_state_dict(cfg, seed=0))
        m.to("cuda").eval()
        x = torch.randn(S, CAP, 3, 224, 224).cuda()
        rows = {"one": [], "a": [], "b": [], "c": []}
        with torch.no_grad():
            for _ in range(REPS):
                rows["one"].append(lockstep(m, x, 1))
                rows["a"].append(lockstep(m, x, S))
                if HAS_RAGGED:
                    rows["b"].append(ragged(m, x))
                rows["c"].append(private(m, x))
        names = {"one": "one stream, one frame      ", "a": "(a) lockstep, 8 streams    ", "b": "(b) ragged, 8 streams      ",
                 "c": "(c) 8 private caches       "}
        for k, v in rows.items():
            if v:
                print(f"[{mode}] {names[k]} p50 ms per call: " + "  ".join(f"{t:.3f}" for t in v) +
                      f"   median {sorted(v)[len(v) // 2]:.3f}  spread {max(v) - min(v):.3f}")
        del m, x


if __name__ == "__main__":
    main()
