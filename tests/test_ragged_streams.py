"""Independent stream positions in one batched KV-cache: ``forward(..., past_key_values=cache, stream_ids=[...])`` advances any
subset of a cache's streams, each from its own position (C ABI: ``sf_forward_stream_slots``).

The oracle is ``O.forward(sd, cfg, x, cache=..., window=...)`` with one private B = 1 oracle cache per stream.  No tolerance is new:
a row's arithmetic in a ragged call is that of the lockstep call with the same number of rows, so the bounds are the constants the
lockstep streaming tests of tests/test_hip_parity.py use for the same model size and mode —

  * small_cfg: ACC_CEIL (fp32-accurate) and BF16_LHS (bf16), on both outputs, as test_sliding_window_cache_outlives_num_frames;
  * head_dim 72: the streamed part of test_forward_head_widths_other_than_64_vs_reference_fixture (8e-5 / BF16_LHS, BF16_POOL);
  * SigLIP-base: test_several_streams_per_call_vs_oracle (9e-5 / BF16_LHS, BF16_POOL).
"""
import pytest
import torch

from oracle import streamformer_oracle as O
from streamformer_amd.configuration import StreamformerConfig, siglip_base
from streamformer_amd.init_weights import make_state_dict
from tests.helpers import frames, maxabs, small_cfg
from tests.test_hip_parity import ACC_CEIL, BF16_LHS, BF16_POOL

SMALL = [("fp32", ACC_CEIL), ("bf16", BF16_LHS)]
HD72W = dict(image_size=42, patch_size=14, num_frames=8, hidden_size=576, num_hidden_layers=2, num_attention_heads=8, intermediate_size=1072)


def build(cfg, sd, mode):
    import streamformer_amd as sa
    assert torch.cuda.is_available(), "these tests need the MI355X"
    m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
    m.load_state_dict(sd)
    return m.to("cuda").eval()


class Stream:
    """One session: its frames, its private oracle cache, how far it has come."""

    def __init__(self, cfg, sd, seed, total, size, window=None):
        self.cfg, self.sd, self.window = cfg, sd, window
        self.x = frames(seed, (1, total, 3, size, size))
        self.ocache = O.new_cache(cfg)
        self.t = 0

    def take(self, T):
        x = self.x[:, self.t:self.t + T]
        assert x.shape[1] == T, "the test's own schedule ran out of frames"
        self.t += T
        return x

    def want(self, x):
        return O.forward(self.sd, self.cfg, x, cache=self.ocache, window=self.window)


def ragged_call(m, cache, sessions, ids, T=1, check=None):
    """One call for the streams `ids` (in that order); returns (last_hidden_state, pooler_output) and, with check=(tol_l, tol_p),
    compares every returned row with its stream's oracle."""
    xs = [sessions[i].take(T) for i in ids]
    out = m(torch.cat(xs, 0).cuda(), past_key_values=cache, stream_ids=list(ids))
    lhs, pool = out.last_hidden_state, out.pooler_output
    assert lhs.shape[:2] == (len(ids), T) and pool.shape[:2] == (len(ids), T)
    if check is not None:
        for row, (i, x) in enumerate(zip(ids, xs)):
            want = sessions[i].want(x)
            dl, dp = maxabs(lhs[row], want["last_hidden_state"][0]), maxabs(pool[row], want["pooler_output"][0])
            print(f"stream {i} at frame {sessions[i].t - T}+{T}: max-abs lhs {dl:.3e} pooler {dp:.3e}")
            assert dl <= check[0] and dp <= check[1], (i, sessions[i].t, dl, dp)
    return lhs, pool


# ------------------------------------------------------------------------------------------------
# 1 + 2b. join, skip, restart, leave
# ------------------------------------------------------------------------------------------------
def join_skip_restart_schedule(m, cache, cfg, sd, check):
    """About ten calls on a cache of three streams; returns every call's outputs."""
    ids = [cache.acquire() for _ in range(3)]
    assert ids == [0, 1, 2]
    with pytest.raises(RuntimeError, match="release"):
        cache.acquire()
    S = {i: Stream(cfg, sd, 100 + i, 12, cfg.image_size) for i in ids}
    seen = [0, 0, 0]
    outs = []

    def call(who, T=1):
        outs.append(ragged_call(m, cache, S, who, T, check))
        for i in who:
            seen[i] += T
        assert cache.frames_seen_per_stream == seen and cache.frames_seen == max(seen)
        assert [cache.get_seq_length(stream=i) for i in ids] == seen

    call([0])                    # stream 0 runs from call 0
    call([0])
    call([1], T=3)               # stream 1 joins with a three-frame prefill ...
    call([0, 1])                 # ... then runs single frames
    call([2, 0, 1])              # stream 2 joins; rows come back in the order asked for
    call([1, 2])                 # stream 0 skips a call
    cache.release(0)             # stream 0 leaves; its slab goes to a new session on different frames
    seen[0] = 0
    assert cache.frames_seen_per_stream == seen
    assert cache.acquire() == 0
    S[0] = Stream(cfg, sd, 200, 12, cfg.image_size)
    call([0, 2])                 # stream 1 skips
    call([0, 1, 2])
    call([2, 1])
    call([0, 1, 2])
    for i in ids:
        cache.release(i)
    assert cache.frames_seen_per_stream == [0, 0, 0]
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol", SMALL)
def test_join_skip_restart_leave_vs_oracle(mode, tol):
    cfg = small_cfg()
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, mode)
    cache = m.new_cache(3, cfg.num_frames)
    first = join_skip_restart_schedule(m, cache, cfg, sd, (tol, tol))
    # the second pass replays captured graphs where the first ran each shape eagerly once: same bits
    second = join_skip_restart_schedule(m, cache, cfg, sd, None)
    assert len(first) == len(second) == 10
    for a, b in zip(first, second):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------
# 2. level streams equal the lockstep call, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_level_streams_equal_lockstep_bit_for_bit(mode):
    cfg = small_cfg()
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, mode)
    B = 3
    x = frames(31, (B, 6, 3, 48, 48)).cuda()
    ragged, lock = m.new_cache(B, cfg.num_frames), m.new_cache(B, cfg.num_frames)
    for t in range(6):
        a = m(x[:, t:t + 1], past_key_values=ragged, stream_ids=range(B), cache_position=torch.full((B,), t))
        b = m(x[:, t:t + 1], use_cache=True, past_key_values=lock)
        assert torch.equal(a.last_hidden_state, b.last_hidden_state), t
        assert torch.equal(a.pooler_output, b.pooler_output), t
    # level again, the lockstep entry points serve the cache the ragged calls filled (and the other way round)
    a = m(x[:, :1], use_cache=True, past_key_values=ragged)
    b = m(x[:, :1], past_key_values=lock, stream_ids=range(B))
    assert torch.equal(a.last_hidden_state, b.last_hidden_state) and torch.equal(a.pooler_output, b.pooler_output)
    assert ragged.frames_seen_per_stream == lock.frames_seen_per_stream == [7] * B


# ------------------------------------------------------------------------------------------------
# 3. one call across the 1-, 2- and 4-pass classes of the single-query attention
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol", SMALL)
def test_mixed_key_pass_classes_graph_and_eager(mode, tol, switches):
    """One layer, num_frames = cap = 132, three streams: one fresh, two prefilled.  Six calls advance all three, so a call holds
    streams of the 1-, 2- and 4-pass classes (the pass count comes from the longest) and the prefilled ones cross 64 and 128 keys.

    The prefills are 60 and 124 frames.  (128 frames, as first written down for this case, leaves room for four more frames under
    cap = 132, not six, and starts past 128 instead of crossing it; 124 puts keys 125..130 into the six calls.)
    Once from the captured graphs and once with SF_DISABLE_STREAM_GRAPH: same bits."""
    cap = 132
    cfg = small_cfg(num_frames=cap, num_hidden_layers=1)
    sd = make_state_dict(cfg, seed=6)
    m = build(cfg, sd, mode)
    prefill = {0: 0, 1: 60, 2: 124}
    runs = []
    for eager in (False, True):
        if eager:
            switches("SF_DISABLE_STREAM_GRAPH")
        cache = m.new_cache(3, cap)
        S = {i: Stream(cfg, sd, 300 + i, prefill[i] + 6, 48) for i in range(3)}
        outs = []
        for i in (1, 2):
            ragged_call(m, cache, S, [i], prefill[i], None if eager else (tol, tol))
        for k in range(6):
            outs.append(ragged_call(m, cache, S, [0, 1, 2], 1, None if eager else (tol, tol)))
            assert cache.frames_seen_per_stream == [k + 1, 61 + k, 125 + k]
        runs.append(outs)
    for a, b in zip(*runs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------
# 4. sliding window per stream
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol", SMALL)
def test_sliding_window_per_stream(mode, tol):
    """policy="slide", cap 6 (time-embedding table of 4 rows): stream 0 runs 2.5 windows deep, stream 1 starts late, so that calls hold
    a wrapped and an unwrapped stream."""
    cap = 6
    cfg = small_cfg(num_frames=4)
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, mode)
    total = int(2.5 * cap) + 1
    late = total - 4
    cache = m.new_cache(2, cap, policy="slide")
    S = {i: Stream(cfg, sd, 400 + i, total, 48, window=cap) for i in range(2)}
    for k in range(total):
        who = [0] if k < late else ([1, 0] if k % 2 else [0, 1])
        ragged_call(m, cache, S, who, 1, (tol, tol))
    assert cache.frames_seen_per_stream == [total, 4]
    assert cache.get_seq_length(stream=0) == cap and cache.get_seq_length(stream=1) == 4 and cache.get_seq_length() == cap


# ------------------------------------------------------------------------------------------------
# 5. generic head width
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol_l,tol_p", [("fp32", 8e-5, 8e-5), ("bf16", BF16_LHS, BF16_POOL)])
def test_generic_head_width_two_positions(mode, tol_l, tol_p):
    cfg = StreamformerConfig(enable_causal_temporal=True, **HD72W)
    sd = make_state_dict(cfg, seed=15)
    m = build(cfg, sd, mode)
    cache = m.new_cache(2, cfg.num_frames)
    S = {i: Stream(cfg, sd, 500 + i, cfg.num_frames, cfg.image_size) for i in range(2)}
    ragged_call(m, cache, S, [1], 3, (tol_l, tol_p))
    for _ in range(4):
        ragged_call(m, cache, S, [0, 1], 1, (tol_l, tol_p))
    ragged_call(m, cache, S, [0], 1, (tol_l, tol_p))
    assert cache.frames_seen_per_stream == [5, 7]


# ------------------------------------------------------------------------------------------------
# 6. SigLIP-base size
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode,tol_l,tol_p", [("fp32", 9e-5, 9e-5), ("bf16", BF16_LHS, BF16_POOL)])
def test_siglip_base_staggered_streams(mode, tol_l, tol_p):
    cfg = siglip_base(num_hidden_layers=3)
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, mode)
    cache = m.new_cache(4, cfg.num_frames)
    S = {i: Stream(cfg, sd, 600 + i, 8, 224) for i in range(4)}
    for i in (1, 2, 3):
        ragged_call(m, cache, S, [i], i, (tol_l, tol_p))
    ragged_call(m, cache, S, [0, 1, 2, 3], 1, (tol_l, tol_p))
    ragged_call(m, cache, S, [0, 1, 2, 3], 1, (tol_l, tol_p))
    ragged_call(m, cache, S, [3, 1], 1, (tol_l, tol_p))
    assert cache.frames_seen_per_stream == [2, 4, 4, 6]


# ------------------------------------------------------------------------------------------------
# 7. refusals say what to do and leave the cache usable
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_cache_usable():
    cfg = small_cfg(num_frames=4)
    sd = make_state_dict(cfg, seed=4)
    m = build(cfg, sd, "fp32")
    cache = m.new_cache(3, 4)
    S = {i: Stream(cfg, sd, 700 + i, 8, 48) for i in range(3)}
    x1 = frames(1, (1, 1, 3, 48, 48)).cuda()
    x2 = frames(2, (2, 1, 3, 48, 48)).cuda()
    x3 = frames(3, (3, 1, 3, 48, 48)).cuda()

    with pytest.raises(Exception, match="named twice"):
        m(x2, past_key_values=cache, stream_ids=[1, 1])
    with pytest.raises(Exception, match=r"ids are 0 \.\. 2"):
        m(x1, past_key_values=cache, stream_ids=[3])
    with pytest.raises(Exception, match=r"ids are 0 \.\. 2"):
        m(x1, past_key_values=cache, stream_ids=[-1])
    with pytest.raises(Exception, match="call once per stream"):
        m(frames(4, (2, 2, 3, 48, 48)).cuda(), past_key_values=cache, stream_ids=[0, 1])
    with pytest.raises(ValueError, match="stream_ids names"):
        m(x2, past_key_values=cache, stream_ids=[0])
    with pytest.raises(NotImplementedError):
        m(x1, past_key_values=cache, stream_ids=[0], output_hidden_states=True)
    assert cache.frames_seen_per_stream == [0, 0, 0]

    ragged_call(m, cache, S, [0], 2, (ACC_CEIL, ACC_CEIL))
    with pytest.raises(ValueError, match="does not continue stream 0"):
        m(x1, past_key_values=cache, stream_ids=[0], cache_position=torch.tensor([0]))
    with pytest.raises(Exception, match="sf_forward_stream_slots"):      # a lockstep call on a ragged cache names the ragged entry point
        m(x3, use_cache=True, past_key_values=cache)
    assert cache.frames_seen_per_stream == [2, 0, 0]

    ragged_call(m, cache, S, [0, 1], 1, (ACC_CEIL, ACC_CEIL))
    ragged_call(m, cache, S, [1, 0], 1, (ACC_CEIL, ACC_CEIL))           # stream 0 is now at capacity (policy "stop")
    with pytest.raises(Exception, match="stream 0 holds 4 of 4 frames.*leave it out"):
        m(x3, past_key_values=cache, stream_ids=[2, 0, 1])
    assert cache.frames_seen_per_stream == [4, 2, 0]                    # nothing was launched for the others either
    ragged_call(m, cache, S, [2, 1], 1, (ACC_CEIL, ACC_CEIL))           # the others still advance in a call that omits it
    cache.reset(0)
    S[0] = Stream(cfg, sd, 710, 8, 48)
    ragged_call(m, cache, S, [0, 1, 2], 1, (ACC_CEIL, ACC_CEIL))
    assert cache.frames_seen_per_stream == [1, 4, 2]

    for _ in range(3):
        cache.acquire()
    with pytest.raises(RuntimeError, match="release"):
        cache.acquire()
    with pytest.raises(ValueError):
        cache.release(3)
    cache.release(1)
    assert cache.frames_seen_per_stream == [1, 0, 2] and cache.acquire() == 1


# ------------------------------------------------------------------------------------------------
# 8. CPU: the free list of slabs
# ------------------------------------------------------------------------------------------------
def test_acquire_release_free_list_on_a_stub():
    from streamformer_amd.modeling import StreamCache

    class Stub(StreamCache):
        def __init__(self, batch):       # no device, no library handle
            self.batch, self._free, self.resets = batch, list(range(batch)), []

        def reset(self, stream=None):
            self.resets.append(stream)

        def __del__(self):
            pass

    c = Stub(3)
    assert [c.acquire(), c.acquire(), c.acquire()] == [0, 1, 2]
    with pytest.raises(RuntimeError, match="all 3 streams.*release"):
        c.acquire()
    c.release(1)
    assert c.resets == [1]                       # release resets the slab
    with pytest.raises(ValueError, match="not acquired"):
        c.release(1)
    for bad in (3, -1, True, "0"):
        with pytest.raises(ValueError):
            c.release(bad)
    assert c.acquire() == 1
    c.release(2)
    c.release(0)
    assert c.acquire() == 0 and c.acquire() == 2         # lowest free slab first
    assert c.resets == [1, 2, 0]


def test_new_entry_points_are_in_the_ctypes_table():
    import streamformer_amd._native as nat
    for name in ("sf_cache_stream_length", "sf_cache_reset_stream", "sf_forward_stream_slots"):
        assert name in nat.SIGNATURES and hasattr(nat.lib, name)
    assert nat.lib.sf_abi_version() == 5
