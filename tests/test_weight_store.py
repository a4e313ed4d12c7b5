"""The staging dtypes of the four native handles, through the C ABI.

The Python wrappers always stage fp32 (the encoder's passes checkpoint dtypes through), so SF_F64 and SF_BF16 are reached only here.
Weights are drawn seeded and rounded to bf16-representable values: fp32, fp64 and bf16 then hold the SAME numbers, every conversion of
the weight store is exact, and three fresh handles loaded from the three forms must produce bitwise equal outputs in both compute
modes: no tolerance.  A handle with one key withheld must refuse to finalize and name the key.

The modules that own such handles copy and pickle like any ``nn.Module``: the copy packs a handle of its own from its own weights."""
import copy
import ctypes as C
import io

import pytest
import torch

import streamformer_amd as sa
from streamformer_amd import _native as nat
from tests.helpers import frames, gpu_device, small_cfg

pytestmark = pytest.mark.gpu

FORMS = {nat.SF_F32: torch.float32, nat.SF_F64: torch.float64, nat.SF_BF16: torch.bfloat16, nat.SF_F16: torch.float16}
COMPUTES = (nat.SF_COMPUTE_BF16, nat.SF_COMPUTE_BF16X3)


def _weights(seed, shapes):
    """name -> seeded fp32 tensor of bf16-representable values; LayerNorm gains (the 1-d "weight"s) sit around 1."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape in shapes.items():
        t = torch.randn(*shape, generator=g) * (0.25 if len(shape) == 1 else 0.08)
        if len(shape) == 1 and k.endswith("weight"):
            t = t + 1.0
        out[k] = t.to(torch.bfloat16).float()
    return out


def _load(load_fn, h, weights, code, skip=None, shape_of=None):
    for k, t in weights.items():
        if k == skip:
            continue
        host = t.to(FORMS[code]).contiguous()
        assert torch.equal(host.double(), t.double()), k          # the form holds the same numbers
        shape = tuple(shape_of(k, host)) if shape_of else tuple(host.shape)
        arr = (C.c_int64 * max(len(shape), 1))(*shape)
        nat.check(load_fn(h, k.encode(), host.data_ptr(), code, arr, len(shape)))


def _ws(bytes_fn, dev, *args):
    n = C.c_size_t()
    nat.check(bytes_fn(*args, C.byref(n)))
    return torch.empty(max(n.value, 256), dtype=torch.uint8, device=dev)


def _same_for_every_form(run, codes=(nat.SF_F32, nat.SF_F64, nat.SF_BF16)):
    """run(code, compute) -> tuple of output tensors; bitwise equal across `codes` in each compute mode."""
    for compute in COMPUTES:
        outs = [run(code, compute) for code in codes]
        for o in outs[0]:
            assert bool(torch.isfinite(o).all()) and float(o.abs().max()) > 0
        for code, other in zip(codes[1:], outs[1:]):
            for a, b in zip(outs[0], other):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (compute, code)


def _refuses_without(create, load_fn, finalize, destroy, weights, key, **kw):
    h = create()
    try:
        _load(load_fn, h, weights, nat.SF_F32, skip=key, **kw)
        assert finalize(h) == nat.SF_ERR_STATE
        msg = (nat.lib.sf_last_error() or b"").decode()
        assert msg.startswith("missing 1 weights: ") and key in msg, msg
    finally:
        destroy(h)


# ------------------------------------------------------------------------------------------------ text tower
def test_text_tower_forms():
    dev = gpu_device()
    V, Pn, D, I, Pr, B, L = 32, 8, 64, 96, 16, 2, 5          # intermediate 96: the zero-padding to 128 is on the path
    shapes = {"embeddings.token_embedding.weight": (V, D), "embeddings.position_embedding.weight": (Pn, D),
              "final_layer_norm.weight": (D,), "final_layer_norm.bias": (D,), "head.weight": (Pr, D), "head.bias": (Pr,)}
    p = "encoder.layers.0."
    for ln in ("layer_norm1", "layer_norm2"):
        shapes[p + ln + ".weight"], shapes[p + ln + ".bias"] = (D,), (D,)
    for a in ("q_proj", "k_proj", "v_proj", "out_proj"):
        shapes[p + "self_attn." + a + ".weight"], shapes[p + "self_attn." + a + ".bias"] = (D, D), (D,)
    shapes.update({p + "mlp.fc1.weight": (I, D), p + "mlp.fc1.bias": (I,), p + "mlp.fc2.weight": (D, I), p + "mlp.fc2.bias": (D,)})
    w = _weights(31, shapes)
    ids = torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(32), dtype=torch.int32).to(dev)
    mask = torch.ones(B, L, dtype=torch.uint8)
    mask[1, 1] = 0                                            # one masked key
    mask = mask.to(dev)
    cfg = nat.SfTextConfig(V, Pn, D, 1, 1, I, Pr, 1, 1e-6)

    def create():
        h = C.c_void_p()
        nat.check(nat.lib.sf_text_create(C.byref(cfg), 0, C.byref(h)))
        return h

    def run(code, compute):
        h = create()
        try:
            _load(nat.lib.sf_text_load_tensor, h, w, code)
            with torch.cuda.device(dev):
                nat.check(nat.lib.sf_text_finalize(h, compute))
                ws = _ws(nat.lib.sf_text_workspace_bytes, dev, h, B, L)
                hid, pooled = torch.zeros(B, L, D, device=dev), torch.zeros(B, Pr, device=dev)
                nat.check(nat.lib.sf_text_forward(h, ids.data_ptr(), mask.data_ptr(), B, L, hid.data_ptr(), pooled.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), nat.current_stream_handle(dev)))
                torch.cuda.synchronize(dev)
            return hid.cpu(), pooled.cpu()
        finally:
            nat.lib.sf_text_destroy(h)

    _same_for_every_form(run)
    _refuses_without(create, nat.lib.sf_text_load_tensor, lambda h: nat.lib.sf_text_finalize(h, nat.SF_COMPUTE_BF16), nat.lib.sf_text_destroy,
                     w, p + "mlp.fc2.bias")


# ------------------------------------------------------------------------------------------------ connector
def test_connector_forms():
    dev = gpu_device()
    Din, Dout, F, P = 64, 128, 1, 4
    w = _weights(41, {"mm_projector.0.weight": (Dout, Din), "mm_projector.0.bias": (Dout,), "mm_projector.2.weight": (Dout, Dout),
                      "mm_projector.2.bias": (Dout,), "image_newline": (Dout,)})
    feats = frames(42, (F, P * P, Din)).to(dev)
    cfg = nat.SfConnectorConfig(Din, Dout, 2, 1, 2, 3)         # mlp2x_gelu, average pool stride 2, newline = grid

    def create():
        h = C.c_void_p()
        nat.check(nat.lib.sf_connector_create(C.byref(cfg), 0, C.byref(h)))
        return h

    def run(code, compute):
        h = create()
        try:
            _load(nat.lib.sf_connector_load_tensor, h, w, code)
            with torch.cuda.device(dev):
                nat.check(nat.lib.sf_connector_finalize(h, compute))
                rows = C.c_int64()
                nat.check(nat.lib.sf_connector_num_tokens(h, F, P, C.byref(rows)))
                assert rows.value == F * 2 * 3
                ws = _ws(nat.lib.sf_connector_workspace_bytes, dev, h, F, P)
                out = torch.zeros(rows.value, Dout, device=dev)
                nat.check(nat.lib.sf_connector_forward(h, feats.data_ptr(), F, P, out.data_ptr(), nat.SF_F32, ws.data_ptr(), ws.numel(),
                                                       nat.current_stream_handle(dev)))
                torch.cuda.synchronize(dev)
            return (out.cpu(),)
        finally:
            nat.lib.sf_connector_destroy(h)

    _same_for_every_form(run)
    _refuses_without(create, nat.lib.sf_connector_load_tensor, lambda h: nat.lib.sf_connector_finalize(h, nat.SF_COMPUTE_BF16),
                     nat.lib.sf_connector_destroy, w, "image_newline")


# ------------------------------------------------------------------------------------------------ detector
def _oad_layer_shapes(p, d, ffn, decoder):
    s = {}
    for a in ("self_attn.",) + (("multihead_attn.",) if decoder else ()):
        s.update({p + a + "in_proj_weight": (3 * d, d), p + a + "in_proj_bias": (3 * d,), p + a + "out_proj.weight": (d, d), p + a + "out_proj.bias": (d,)})
    s.update({p + "linear1.weight": (ffn, d), p + "linear1.bias": (ffn,), p + "linear2.weight": (d, ffn), p + "linear2.bias": (d,)})
    for n in ("norm1.", "norm2.") + (("norm3.",) if decoder else ()):
        s.update({p + n + "weight": (d,), p + n + "bias": (d,)})
    return s


def test_detector_forms():
    dev = gpu_device()
    d, heads, ffn, L, W, classes, Q0, pe_rows = 64, 2, 64, 4, 2, 3, 2, 8      # classes 3: the classifier's padding to 16 rows is on the path
    shapes = {}
    for fh in ("feature_head_long.", "feature_head_work."):
        shapes.update({fh + "visual_linear.0.weight": (d, d), fh + "visual_linear.0.bias": (d,), fh + "visual_linear.1.weight": (d,),
                       fh + "visual_linear.1.bias": (d,)})
    shapes["enc_queries.0.weight"] = (Q0, d)
    shapes.update(_oad_layer_shapes("enc_modules.0.layers.0.", d, ffn, True))
    shapes.update({"enc_modules.0.norm.weight": (d,), "enc_modules.0.norm.bias": (d,)})
    shapes.update(_oad_layer_shapes("dec_modules.layers.0.", d, ffn, True))
    shapes.update({"dec_modules.norm.weight": (d,), "dec_modules.norm.bias": (d,), "classifier.weight": (classes, d), "classifier.bias": (classes,)})
    shapes["pos_encoding.pe"] = (pe_rows, d)
    w = _weights(51, shapes)
    pe_as_buffer = lambda k, host: (pe_rows, 1, d) if k == "pos_encoding.pe" else host.shape      # the reference's [max_len, 1, d]; L + W rows are kept
    work = [frames(52 + i, (1, W, d)).to(dev) for i in range(3)]
    longs = [frames(56, (L, d)).to(dev), frames(57, (1, d)).to(dev), None]      # the whole window, one new sample, the cached memory
    cfg = nat.SfOadConfig()
    cfg.d_in, cfg.d_model, cfg.heads, cfg.ffn, cfg.long_samples, cfg.work_samples, cfg.classes = d, d, heads, ffn, L, W, classes
    cfg.act, cfg.linear_enabled, cfg.enc_modules = 2, 1, 1
    cfg.enc_queries[0], cfg.enc_layers[0], cfg.enc_norm[0] = Q0, 1, 1
    cfg.dec_layers, cfg.dec_norm, cfg.eps = 1, 1, 1e-5

    def create():
        h = C.c_void_p()
        nat.check(nat.lib.sf_oad_create(C.byref(cfg), 0, C.byref(h)))
        return h

    def run(code, compute):
        h, st = create(), C.c_void_p()
        try:
            _load(nat.lib.sf_oad_load_tensor, h, w, code, shape_of=pe_as_buffer)
            outs = []
            with torch.cuda.device(dev):
                nat.check(nat.lib.sf_oad_finalize(h, compute))
                nat.check(nat.lib.sf_oad_state_create(h, 1, C.byref(st)))
                ws = _ws(nat.lib.sf_oad_workspace_bytes, dev, h, 1)
                ids = (C.c_int32 * 1)(0)
                for x, lm in zip(work, longs):
                    rows = (C.c_int32 * 1)(0 if lm is None else lm.shape[0])
                    out = torch.zeros(1, W, classes, device=dev)
                    nat.check(nat.lib.sf_oad_step(h, st, ids, 1, x.data_ptr(), nat.ptr(lm), rows, None, out.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                                                  nat.current_stream_handle(dev)))
                    torch.cuda.synchronize(dev)
                    outs.append(out.cpu())
            return tuple(outs)
        finally:
            if st:
                nat.lib.sf_oad_state_destroy(st)
            nat.lib.sf_oad_destroy(h)

    _same_for_every_form(run)
    _refuses_without(create, nat.lib.sf_oad_load_tensor, lambda h: nat.lib.sf_oad_finalize(h, nat.SF_COMPUTE_BF16), nat.lib.sf_oad_destroy, w,
                     "dec_modules.layers.0.norm3.bias", shape_of=pe_as_buffer)


# ------------------------------------------------------------------------------------------------ encoder
def test_encoder_forms():
    dev = gpu_device()
    cfg = small_cfg()                                          # the smallest encoder the parity tests build
    m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype="bf16")
    m.load_state_dict(sa.make_state_dict(cfg, seed=61))
    named = {k: p.detach().float().cpu() for k, p in m._named.items()}
    sfc = m._sf_config()
    B, T, N, D = 1, cfg.num_frames, cfg.num_patches, cfg.hidden_size
    x = frames(62, (B, T, 3, cfg.image_size, cfg.image_size)).to(dev)      # one clip

    def create():
        h = C.c_void_p()
        nat.check(nat.lib.sf_create(C.byref(sfc), 0, C.byref(h)))
        return h

    def runner(w):
        def run(code, compute):
            h = create()
            try:
                _load(nat.lib.sf_load_tensor, h, w, code)
                with torch.cuda.device(dev):
                    nat.check(nat.lib.sf_finalize_weights(h, compute, 1, 0))
                    ws = _ws(nat.lib.sf_workspace_bytes, dev, h, B, T, cfg.image_size, cfg.image_size)
                    hid, pool = torch.zeros(B, T, N, D, device=dev), torch.zeros(B, T, D, device=dev)
                    nat.check(nat.lib.sf_forward(h, x.data_ptr(), nat.SF_F32, B, T, cfg.image_size, cfg.image_size, hid.data_ptr(), pool.data_ptr(),
                                                 None, None, ws.data_ptr(), ws.numel(), nat.current_stream_handle(dev)))
                    torch.cuda.synchronize(dev)
                return hid.cpu(), pool.cpu()
            finally:
                nat.lib.sf_destroy(h)
        return run

    _same_for_every_form(runner({k: t.to(torch.bfloat16).float() for k, t in named.items()}))
    # fp16-representable values: SF_F16 (which only the encoder takes) against the same values as fp32
    _same_for_every_form(runner({k: t.to(torch.float16).float() for k, t in named.items()}), codes=(nat.SF_F32, nat.SF_F16))
    w = {k: t.to(torch.bfloat16).float() for k, t in named.items()}
    _refuses_without(create, nat.lib.sf_load_tensor, lambda h: nat.lib.sf_finalize_weights(h, nat.SF_COMPUTE_BF16, 1, 0), nat.lib.sf_destroy, w,
                     "encoder.layer.1.output.dense.weight")


# ------------------------------------------------------------------------------------------------ copies of the owning modules
def _copies(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return copy.deepcopy(m), torch.load(buf, weights_only=False)


def _bits(t):          # fp32 bit patterns; helpers.bf16_bits is the bf16 rounding
    return t.detach().cpu().view(torch.int32)


def test_text_tower_copies():
    dev = gpu_device()
    torch.manual_seed(71)
    m = sa.SiglipTextModel(sa.SiglipTextConfig(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                               max_position_embeddings=8), device=dev)
    ids = torch.randint(0, 32, (2, 4), generator=torch.Generator().manual_seed(72)).to(dev)
    want = [_bits(t) for t in m(ids)]
    assert m._handle is not None and float(m(ids)[1].abs().max()) > 0
    for other in _copies(m):
        assert other._handle is None and other._native is not m._native       # an empty owner: nothing of the original's is shared
        assert all(torch.equal(a, _bits(b)) for a, b in zip(want, other(ids)))
        with torch.no_grad():
            other.embeddings.token_embedding.weight.add_(0.5)
        assert not any(torch.equal(a, _bits(b)) for a, b in zip(want, other(ids)))
        assert all(torch.equal(a, _bits(b)) for a, b in zip(want, m(ids)))    # the edit reached the copy alone


def test_connector_copies():
    dev = gpu_device()
    torch.manual_seed(73)
    F, P = 2, 4
    m = sa.VideoTokenConnector(dict(mm_projector_type="mlp2x_gelu", mm_hidden_size=64, hidden_size=64, mm_spatial_pool_stride=2), device=dev)
    feats = frames(74, (F, P * P, 64)).to(dev)
    want = _bits(m(feats))
    rows = m.num_tokens(F, P)
    assert want.shape == (rows, 64) and float(m(feats).abs().max()) > 0
    for other in _copies(m):
        assert other._probes == {} and other._native.handles == {}
        assert other.num_tokens(F, P) == rows                                 # the copy makes probes of its own
        assert torch.equal(want, _bits(other(feats)))
        assert torch.equal(_bits(m.layout(m.project_frames(feats))), _bits(other.layout(other.project_frames(feats))))
        with torch.no_grad():
            other.mm_projector[2].bias.add_(0.5)
        assert not torch.equal(want, _bits(other(feats)))
        assert torch.equal(want, _bits(m(feats)))


def test_detector_copies():
    dev = gpu_device()
    torch.manual_seed(75)
    d, L, W = 64, 4, 2                                        # the config of test_detector_forms
    m = sa.OnlineActionDetector(sa.OADConfig(VISUAL_SIZE=d, NUM_CLASSES=3, LINEAR_OUT_FEATURES=d, NUM_HEADS=2, DIM_FEEDFORWARD=64,
                                             LONG_MEMORY_NUM_SAMPLES=L, WORK_MEMORY_NUM_SAMPLES=W, ENC_MODULE=[[2, 1, True]],
                                             DEC_MODULE=[-1, 1, True]), device=dev)
    work, long = frames(76, (1, W, d)).to(dev), frames(77, (L, d)).to(dev)
    state = m.new_state(1)
    want = _bits(m.step(work, [long], state=state))
    assert float(want.float().abs().max()) > 0
    for other in _copies(m):
        assert other._native.handles == {} and other._native.token is None
        assert torch.equal(want, _bits(other.step(work, [long], state=other.new_state(1))))
        with pytest.raises(ValueError, match="this state belongs to another detector"):
            other.step(work, None, state=state)
    with pytest.raises(TypeError, match="a DetectorState is device memory of one native handle and cannot be copied or pickled"):
        copy.deepcopy(state)
    assert state.fill(0) == L                                 # refused, not harmed
