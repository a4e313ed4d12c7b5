"""Parking one SigLIP-base stream (224^2 frames, 64-frame cache): how fast its K/V leave the slab and come back.

For 16 and 64 cached frames, in both compute modes:

  export     sf_cache_export_stream into a preallocated device blob (one launch), HIP events around ITERS back-to-back calls
  import     sf_cache_import_stream of that blob into the other slab of the cache, the same way
  copy       a plain device-to-device copy (Tensor.copy_) of the same byte count, the same way: the yardstick of the same run
  snapshot / restore            StreamCache.snapshot(0) / .restore(snap, 1) on the device, wall clock to a synchronise (allocation included)
  snapshot cpu / restore cpu    the host round trip: snapshot(0, device="cpu") into pinned memory, restore from it

GB/s = blob bytes per second of the call (every byte is read once and written once, so the memory traffic is twice that), the
same convention for the kernels and the plain copy.  Every quantity is the median of REPS (3) measurements after one warm-up; the
spread is printed.  After the timed imports the slab is exported again and compared with the blob, byte for byte.

    python tools/stream_park.py [--out profiles/stream_park.txt]      SF_MODES=bf16,fp32  SF_REPS=3  SF_ITERS=20"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, streamformer_amd as sa
import streamformer_amd._native as nat

CAP = 64
REPS = int(os.environ.get("SF_REPS", "3"))
ITERS = int(os.environ.get("SF_ITERS", "20"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def device_ms(fn):
    """Mean milliseconds of ITERS back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(v):
    return sorted(v)[len(v) // 2]


def report(mode, k, name, ms, nbytes, base=None):
    m = med(ms)
    rate = nbytes / (m * 1e-3) / 1e9
    tail = "" if base is None else f"   {100 * base / m:5.1f} % of the plain copy's rate"
    say(f"[{mode}] {k:2d} frames  {name:<14s} {m:9.3f} ms  {rate:8.1f} GB/s   spread {max(ms) - min(ms):.3f} ms{tail}")
    return m


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "stream_park.txt")
    cfg = sa.siglip_base(num_frames=CAP)
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {ITERS} calls per measurement, median of {REPS}")
    for mode in os.environ.get("SF_MODES", "bf16,fp32").split(","):
        m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
        m.load_state_dict(sa.make_state_dict(cfg, seed=0))
        m.to("cuda").eval()
        stream = nat.current_stream_handle(m.device)
        x = torch.randn(1, 16, 3, 224, 224).cuda()
        cache = m.new_cache(2, CAP)
        for k in (16, 64):
            with torch.no_grad():
                while cache.frames_seen_per_stream[0] < k:
                    m(x, past_key_values=cache, stream_ids=[0])          # 16-frame prefills
            snap = cache.snapshot(0)
            n = snap.nbytes
            blob, other = snap.blob, torch.empty_like(snap.blob)
            meta = nat.SfCacheStreamMeta(**snap.meta)
            say(f"[{mode}] {k:2d} frames  blob {n / 2**20:.1f} MiB of a {cache.nbytes / 2 / 2**20:.1f} MiB slab")

            def export():
                nat.check(nat.lib.sf_cache_export_stream(m._handle, cache._h, 0, other.data_ptr(), n, ctypes.byref(meta), stream))

            def import_():
                nat.check(nat.lib.sf_cache_import_stream(m._handle, cache._h, 1, blob.data_ptr(), n, ctypes.byref(meta), stream))

            t = {key: [] for key in ("copy", "export", "import", "snapshot", "restore", "snapshot cpu", "restore cpu")}
            for _ in range(REPS):      # the quantities alternate inside a repetition, so drift hits them alike
                t["copy"].append(device_ms(lambda: other.copy_(blob)))
                t["export"].append(device_ms(export))
                t["import"].append(device_ms(import_))
                t["snapshot"].append(wall_ms(lambda: cache.snapshot(0))[0])
                t["restore"].append(wall_ms(lambda: cache.restore(snap, stream=1))[0])
                ms, host = wall_ms(lambda: cache.snapshot(0, device="cpu"))
                t["snapshot cpu"].append(ms)
                t["restore cpu"].append(wall_ms(lambda: cache.restore(host, stream=1))[0])
                del host
            base = report(mode, k, "copy", t["copy"], n)
            for key in ("export", "import"):
                report(mode, k, key, t[key], n, base)
            for key in ("snapshot", "restore", "snapshot cpu", "restore cpu"):
                report(mode, k, key, t[key], n)
            back = cache.snapshot(1)
            assert back.meta == snap.meta and torch.equal(back.blob, blob), "slab 1 does not hold what was imported"
            say(f"[{mode}] {k:2d} frames  slab 1 exported again: identical to the blob")
            del snap, blob, other, back
        del m, cache, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
