"""Parking a stream: ``StreamCache.snapshot()`` packs one stream's cached K/V into a blob, ``StreamCache.restore()`` puts it back
into any slab of any cache of the same model (C ABI: ``sf_cache_export_stream`` / ``sf_cache_import_stream``).

Resumption is checked with ``torch.equal``: the restored frames sit in the ring slots they came from and the frame count is
restored, so the next call's arithmetic is the uninterrupted stream's.  (A row's bits depend on the number of rows of its call —
another row count selects other GEMM kernels — so every comparison pairs calls of the same shape.)

The one comparison against the CPU oracle uses the bounds of the streaming-versus-oracle tests of tests/test_hip_parity.py for
small_cfg (test_sliding_window_cache_outlives_num_frames): ACC_CEIL in the fp32-accurate mode, BF16_LHS in bf16, on both outputs.
"""
import ctypes
import os
import pickle
import re

import pytest
import torch

from oracle import streamformer_oracle as O
from streamformer_amd.init_weights import make_state_dict
from tests.conftest import ROOT
from tests.helpers import frames, maxabs, small_cfg
from tests.test_hip_parity import ACC_CEIL, BF16_LHS

MODES = ["fp32", "bf16"]
NEW_SYMBOLS = ("sf_cache_stream_blob_bytes", "sf_cache_export_stream", "sf_cache_import_stream")


def build(cfg, sd, mode):
    import streamformer_amd as sa
    assert torch.cuda.is_available(), "these tests need the MI355X"
    m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
    m.load_state_dict(sd)
    return m.to("cuda").eval()


def step(m, cache, ids, x):
    """One call for the streams `ids`; x [len(ids), T, 3, H, W].  Returns (last_hidden_state, pooler_output)."""
    o = m(x.cuda(), past_key_values=cache, stream_ids=list(ids))
    return o.last_hidden_state, o.pooler_output


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def feed(m, cache, sid, x, chunks):
    """Stream `sid` takes the frames of x [1, sum(chunks), ...] in calls of `chunks` frames; returns the outputs per call."""
    outs, t = [], 0
    for c in chunks:
        outs.append(step(m, cache, [sid], x[:, t:t + c]))
        t += c
    assert t == x.shape[1]
    return outs


# ------------------------------------------------------------------------------------------------
# 1. bit-identical resumption in another slab
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("before", [[1, 1, 1, 1], [3, 1]], ids=["single-frames", "prefill"])
def test_resumed_stream_is_bit_identical(mode, before):
    """A runs 7 frames uninterrupted.  B runs 4 (as single frames, or a 3-frame prefill and one), is parked, releases its slab,
    comes back in a slab nothing was ever written to, and runs frames 5-7."""
    cfg = small_cfg()
    m = build(cfg, make_state_dict(cfg, seed=4), mode)
    x = frames(51, (1, 7, 3, 48, 48))
    ca = m.new_cache(2, cfg.num_frames)
    a = feed(m, ca, ca.acquire(), x, before + [1, 1, 1])[-3:]
    cb = m.new_cache(3, cfg.num_frames)
    b0 = cb.acquire()
    feed(m, cb, b0, x[:, :4], before)
    snap = cb.snapshot(b0)
    assert snap.frames_seen == 4 and snap.blob.is_cuda
    b1 = cb.acquire()
    cb.release(b0)
    assert b1 != b0 and cb.frames_seen_per_stream == [0, 0, 0]
    assert cb.restore(snap, stream=b1) == b1
    assert cb.frames_seen_per_stream[b1] == 4
    b = feed(m, cb, b1, x[:, 4:], [1, 1, 1])
    for t, (u, v) in enumerate(zip(a, b)):
        assert same(u, v), f"frame {5 + t} differs after the restore: lhs {maxabs(u[0], v[0]):.3e} pooler {maxabs(u[1], v[1]):.3e}"


# ------------------------------------------------------------------------------------------------
# 2. another cache, through host memory and a file
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_host_round_trip_into_another_cache(mode, tmp_path):
    import streamformer_amd as sa
    cfg = small_cfg()
    m = build(cfg, make_state_dict(cfg, seed=4), mode)
    x = frames(52, (1, 7, 3, 48, 48))
    src = m.new_cache(1, cfg.num_frames)
    feed(m, src, 0, x[:, :4], [1] * 4)
    snap = src.snapshot(0, device="cpu")
    assert snap.blob.device.type == "cpu" and snap.blob.is_pinned() and snap.nbytes > 0
    assert snap.to("cuda").blob.is_cuda and snap.to("cpu") is snap
    torch.save(snap, tmp_path / "snap.pt")
    loaded = torch.load(tmp_path / "snap.pt", weights_only=False)
    assert isinstance(loaded, sa.StreamSnapshot) and loaded.meta == snap.meta and torch.equal(loaded.blob, snap.blob)
    torch.save(snap.state_dict(), tmp_path / "plain.pt")
    plain = sa.StreamSnapshot.from_state_dict(torch.load(tmp_path / "plain.pt", weights_only=True))
    want = feed(m, src, 0, x[:, 4:], [1] * 3)              # the source was left as it was: it IS the uninterrupted stream
    dst = m.new_cache(4, cfg.num_frames)
    held = [dst.acquire() for _ in range(2)]
    sid = dst.restore(loaded)
    assert sid == 2 and sid not in held and dst.frames_seen_per_stream == [0, 0, 4, 0]
    got = feed(m, dst, sid, x[:, 4:], [1] * 3)
    other = m.new_cache(2, cfg.num_frames)
    got2 = feed(m, other, other.restore(plain), x[:, 4:], [1] * 3)
    for u, v, w in zip(want, got, got2):
        assert same(u, v) and same(u, w)


# ------------------------------------------------------------------------------------------------
# 3. a sliding window that has wrapped
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_wrapped_sliding_window_resumes_bit_identical(mode):
    """cap 6 over a time-embedding table of 4 rows; parked after 9 frames: the ring has wrapped (next slot 3) and the frames are
    past the table.  The ring is restored slot for slot, not linearised."""
    cap = 6
    cfg = small_cfg(num_frames=4)
    m = build(cfg, make_state_dict(cfg, seed=4), mode)
    x = frames(53, (1, 14, 3, 48, 48))
    src = m.new_cache(1, cap, policy="slide")
    feed(m, src, 0, x[:, :9], [3] + [1] * 6)
    snap = src.snapshot(0)
    assert snap.frames_seen == 9 and snap.meta["frames_held"] == cap
    dst = m.new_cache(3, cap, policy="slide")
    sid = dst.restore(snap, stream=2)
    assert dst.frames_seen_per_stream[sid] == src.frames_seen_per_stream[0] == 9
    assert dst.get_seq_length(stream=sid) == src.get_seq_length(stream=0) == cap
    want = feed(m, src, 0, x[:, 9:], [1] * 5)
    got = feed(m, dst, sid, x[:, 9:], [1] * 5)
    for t, (u, v) in enumerate(zip(want, got)):
        assert same(u, v), 9 + t
    assert dst.frames_seen_per_stream[sid] == src.frames_seen_per_stream[0] == 14


# ------------------------------------------------------------------------------------------------
# 4. fork, next to live neighbours
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fork_between_live_neighbours(mode):
    """Slabs 0 and 1 hold live streams at 2 and 5 frames.  One snapshot (3 frames) goes into slabs 2 and 3; the four streams then
    share calls.  The control cache has the same neighbours and, in slabs 2 and 3, the forked stream run uninterrupted."""
    cfg = small_cfg()
    m = build(cfg, make_state_dict(cfg, seed=4), mode)
    xn = {0: frames(60, (1, 4, 3, 48, 48)), 1: frames(61, (1, 7, 3, 48, 48))}
    xf = frames(62, (1, 5, 3, 48, 48))
    caches = {k: m.new_cache(4, cfg.num_frames) for k in ("forked", "control")}
    for c in caches.values():
        assert [c.acquire() for _ in range(2)] == [0, 1]
        feed(m, c, 0, xn[0][:, :2], [1] * 2)
        feed(m, c, 1, xn[1][:, :5], [1] * 5)
    src = m.new_cache(1, cfg.num_frames)
    feed(m, src, 0, xf[:, :3], [1] * 3)
    snap = src.snapshot(0)
    forks = [caches["forked"].restore(snap), caches["forked"].restore(snap)]
    assert forks == [2, 3] and caches["forked"].frames_seen_per_stream == [2, 5, 3, 3]
    for sid in (2, 3):
        assert caches["control"].acquire() == sid
        feed(m, caches["control"], sid, xf[:, :3], [1] * 3)
    for k in range(2):
        rows = torch.cat([xn[0][:, 2 + k:3 + k], xf[:, 3 + k:4 + k], xf[:, 3 + k:4 + k], xn[1][:, 5 + k:6 + k]], 0)
        got = step(m, caches["forked"], [0, 2, 3, 1], rows)
        want = step(m, caches["control"], [0, 2, 3, 1], rows)
        for out_g, out_w in zip(got, want):
            assert torch.equal(out_g[1], out_g[2]), "the two forks differ"
            assert torch.equal(out_g[1], out_w[1]), "a fork differs from the uninterrupted stream"
            assert torch.equal(out_g[0], out_w[0]) and torch.equal(out_g[3], out_w[3]), "a neighbour saw the restore"
    assert caches["forked"].frames_seen_per_stream == caches["control"].frames_seen_per_stream == [4, 7, 5, 5]


# ------------------------------------------------------------------------------------------------
# 5. against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol", [("fp32", ACC_CEIL), ("bf16", BF16_LHS)])
def test_resumed_stream_vs_oracle(mode, tol):
    cfg = small_cfg()
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, mode)
    x = frames(54, (1, 6, 3, 48, 48))
    src = m.new_cache(2, cfg.num_frames)
    feed(m, src, src.acquire(), x[:, :3], [1] * 3)
    snap = src.snapshot(0)
    del src
    dst = m.new_cache(2, cfg.num_frames)
    dst.acquire()
    sid = dst.restore(snap)
    assert sid == 1
    ocache = O.new_cache(cfg)
    O.forward(sd, cfg, x[:, :3], cache=ocache)
    for t in range(3, 6):
        want = O.forward(sd, cfg, x[:, t:t + 1], cache=ocache)
        lhs, pool = step(m, dst, [sid], x[:, t:t + 1])
        dl, dp = maxabs(lhs, want["last_hidden_state"]), maxabs(pool, want["pooler_output"])
        print(f"{mode} frame {t + 1}: max-abs lhs {dl:.3e} pooler {dp:.3e} (bound {tol:.1e})")
        assert dl <= tol and dp <= tol, (t, dl, dp)


# ------------------------------------------------------------------------------------------------
# 6. the blob holds live frames only
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_blob_holds_only_live_frames(mode):
    """At k frames the blob is at most the stream's share of the cache, k / max_frames of a slab, plus HEADER bytes.  HEADER = 256
    allows for alignment padding of a blob format; the metadata travels next to the blob, not inside it."""
    HEADER = 256
    cfg = small_cfg()
    m = build(cfg, make_state_dict(cfg, seed=4), mode)
    batch, cap = 3, cfg.num_frames
    cache = m.new_cache(batch, cap)
    x = frames(55, (1, 5, 3, 48, 48))
    sizes = [cache.snapshot(1).nbytes]
    assert sizes == [0]
    for k in range(1, 6):
        step(m, cache, [1], x[:, k - 1:k])
        snap = cache.snapshot(1)
        assert snap.nbytes == snap.blob.numel() == snap.meta["blob_bytes"]
        assert 0 < snap.nbytes <= cache.nbytes / batch * k / cap + HEADER, (k, snap.nbytes)
        assert snap.nbytes > sizes[-1]
        sizes.append(snap.nbytes)
    assert cache.snapshot(0).nbytes == 0 and cache.frames_seen_per_stream == [0, 5, 0]


# ------------------------------------------------------------------------------------------------
# 7. refusals leave the destination untouched
# ------------------------------------------------------------------------------------------------
def parked(m, max_frames, policy="stop", size=48, n=3, seed=70):
    c = m.new_cache(1, max_frames, size, size, policy=policy)
    feed(m, c, 0, frames(seed, (1, n, 3, size, size)), [1] * n)
    return c.snapshot(0)


@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched():
    import streamformer_amd as sa
    import streamformer_amd._native as nat
    cfg = small_cfg()
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, "fp32")
    y = frames(71, (1, 3, 3, 48, 48))

    def live_pair(model):
        """Destination and control: slab 0 of both holds the same live stream of 2 frames, slab 1 is free."""
        pair = [model.new_cache(2, cfg.num_frames) for _ in range(2)]
        for c in pair:
            assert c.acquire() == 0
            feed(model, c, 0, y[:, :2], [1] * 2)
        return pair

    def refused(dst, snap, exc, word, stream=0):
        with pytest.raises(exc, match=word) as ei:
            dst.restore(snap, stream=stream)
        print(f"refused ({word}): {ei.value}")
        assert dst.frames_seen_per_stream == [2, 0] and dst._free == [1]

    dst, ctl = live_pair(m)
    good = parked(m, cfg.num_frames)
    refused(dst, parked(m, 8), nat.NativeError, "max_frames")
    refused(dst, parked(m, cfg.num_frames, policy="slide"), nat.NativeError, "policy")
    refused(dst, parked(m, cfg.num_frames, size=32), nat.NativeError, "resolution")
    refused(dst, parked(build(cfg, sd, "bf16"), cfg.num_frames), nat.NativeError, "compute mode")
    refused(dst, parked(build(cfg, make_state_dict(cfg, seed=5), "fp32"), cfg.num_frames), nat.NativeError, "other weights")
    short = sa.StreamSnapshot(good.blob, good.meta)
    short.blob = good.blob[:-16]
    refused(dst, short, ValueError, "truncated")
    # the library's own count check, under the Python one
    meta = nat.SfCacheStreamMeta(**good.meta)
    rc = nat.lib.sf_cache_import_stream(m._handle, dst._h, 0, good.blob.data_ptr(), good.nbytes - 16, ctypes.byref(meta), None)
    assert rc == nat.SF_ERR_INVALID and b"byte count" in nat.lib.sf_last_error()
    assert dst.frames_seen_per_stream == [2, 0]
    for bad in (2, -1):
        refused(dst, good, ValueError, "stream must be", stream=bad)
        assert nat.lib.sf_cache_import_stream(m._handle, dst._h, bad, good.blob.data_ptr(), good.nbytes, ctypes.byref(meta), None) == nat.SF_ERR_INVALID
        assert b"stream" in nat.lib.sf_last_error()
    # stream=None: a refused import hands the slab it acquired back
    refused(dst, parked(m, 8), nat.NativeError, "max_frames", stream=None)
    assert dst.acquire() == 1
    with pytest.raises(RuntimeError, match="in use"):         # a full cache
        dst.restore(good)
    assert dst.frames_seen_per_stream == [2, 0] and dst._free == []
    assert same(step(m, dst, [0], y[:, 2:3]), step(m, ctl, [0], y[:, 2:3])), "a refused restore changed the live stream"
    # a snapshot taken before the model re-packs: the wording of a stale cache
    m.load_state_dict(make_state_dict(cfg, seed=6))
    dst, ctl = live_pair(m)
    refused(dst, good, RuntimeError, "re-packed")
    with pytest.raises(RuntimeError, match="re-packed"):
        ctl.restore(good, stream=None)
    assert ctl._free == [1]
    assert same(step(m, dst, [0], y[:, 2:3]), step(m, ctl, [0], y[:, 2:3]))
    m.set_compute_dtype("bf16")
    with pytest.raises(RuntimeError, match="re-packed"):      # the pending re-pack happens inside restore(): the cache itself is stale
        dst.restore(good, stream=1)


# ------------------------------------------------------------------------------------------------
# 8. ABI (CPU)
# ------------------------------------------------------------------------------------------------
def test_park_entry_points_are_declared_bound_and_exported():
    import streamformer_amd._native as nat
    header = open(os.path.join(ROOT, "include", "streamformer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), f"{s} is not declared in the header"
        assert s in nat.SIGNATURES and hasattr(lib, s)
    assert "sf_cache_stream_meta" in code and "SF_STREAM_BLOB_KV1" in code
    assert nat.lib.sf_abi_version() == 5
    # the ctypes mirror of sf_cache_stream_meta: twelve 32-bit fields, then two 64-bit ones
    assert ctypes.sizeof(nat.SfCacheStreamMeta) == 64 and nat.SfCacheStreamMeta.packing.offset == 48
    assert int(re.search(r"#define\s+SF_STREAM_BLOB_KV1\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == nat.SF_STREAM_BLOB_KV1
    # argument checks that need no device
    n = ctypes.c_size_t()
    assert nat.lib.sf_cache_stream_blob_bytes(None, 0, ctypes.byref(n)) == nat.SF_ERR_INVALID
    meta = nat.SfCacheStreamMeta()
    assert nat.lib.sf_cache_import_stream(None, None, 0, None, 0, ctypes.byref(meta), None) == nat.SF_ERR_INVALID
    assert nat.lib.sf_cache_export_stream(None, None, 0, None, 0, ctypes.byref(meta), None) == nat.SF_ERR_INVALID


# ------------------------------------------------------------------------------------------------
# 9. StreamSnapshot without a device (CPU)
# ------------------------------------------------------------------------------------------------
def cpu_snapshot(seen=5, cap=4, compute=1):
    import streamformer_amd as sa
    import streamformer_amd._native as nat
    L, N, D, esz = 2, 9, 128, 4 if compute == 1 else 2
    held = min(seen, cap)
    n = L * held * N * 2 * D * esz
    meta = dict(format=nat.SF_STREAM_BLOB_KV1, compute=compute, frames_seen=seen, frames_held=held, max_frames=cap, policy=1, H=48,
                W=48, layers=L, hidden_size=D, patches=N, elem_bytes=esz, packing=0xfeedfacecafebeef, blob_bytes=n)
    blob = (torch.arange(n, dtype=torch.int64) % 251).to(torch.uint8)
    return sa.StreamSnapshot(blob, meta), meta, blob


def test_snapshot_is_plain_data(tmp_path):
    import streamformer_amd as sa
    snap, meta, blob = cpu_snapshot()
    assert snap.nbytes == blob.numel() and snap.frames_seen == 5 and snap.device.type == "cpu"
    assert snap.to("cpu") is snap and "frames_seen=5" in repr(snap)
    again = pickle.loads(pickle.dumps(snap))
    assert isinstance(again, sa.StreamSnapshot) and again.meta == meta and torch.equal(again.blob, blob) and again._origin is None
    torch.save(snap, tmp_path / "s.pt")
    loaded = torch.load(tmp_path / "s.pt", weights_only=False)
    assert loaded.meta == meta and torch.equal(loaded.blob, blob)
    torch.save(snap.state_dict(), tmp_path / "p.pt")
    plain = torch.load(tmp_path / "p.pt", weights_only=True)       # nothing but a tensor and a dict of ints
    assert set(plain) == {"blob", "meta"} and all(type(v) is int for v in plain["meta"].values())
    back = sa.StreamSnapshot.from_state_dict(plain)
    assert back.meta == meta and torch.equal(back.blob, blob)
    import streamformer_amd._native as nat
    assert set(meta) == {n for n, _ in nat.SfCacheStreamMeta._fields_}      # the dict mirrors sf_cache_stream_meta field for field


def test_snapshot_metadata_is_validated():
    import streamformer_amd as sa
    _, meta, blob = cpu_snapshot()

    def bad(word, blob_=blob, **change):
        m = dict(meta)
        m.update(change)
        with pytest.raises(ValueError, match=word):
            sa.StreamSnapshot(blob_, m)

    bad("format", format=7)
    bad("frames_held", frames_held=3)
    bad("frames_held", frames_seen=2)
    bad("blob_bytes", layers=3)
    bad("blob_bytes", blob_bytes=meta["blob_bytes"] - 16)
    bad("elem_bytes", elem_bytes=2)
    bad("compute", compute=2)
    bad("non-negative int", policy=-1)
    bad("non-negative int", H=48.0)
    bad("non-negative int", W=True)
    bad("truncated", blob_=blob[:-16])
    bad("uint8", blob_=blob.float())
    bad("1-D", blob_=blob.reshape(2, -1))
    missing = dict(meta)
    del missing["packing"]
    with pytest.raises(ValueError, match="packing"):
        sa.StreamSnapshot(blob, missing)
    with pytest.raises(ValueError, match="extra"):
        sa.StreamSnapshot(blob, dict(meta, extra=1))
    # a pickle that was tampered with is refused on load
    snap, _, _ = cpu_snapshot()
    snap.meta["frames_seen"] = 1
    with pytest.raises(ValueError, match="frames_held"):
        pickle.loads(pickle.dumps(snap))
    with pytest.raises(TypeError, match="StreamSnapshot"):
        sa.StreamCache.restore(object.__new__(sa.StreamCache), {"blob": blob, "meta": meta})
