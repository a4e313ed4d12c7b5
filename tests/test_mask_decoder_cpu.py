"""CPU: the mask decoder's fp64 restatement against fixture F24 (the reference's own two classes), the modules' parameter trees against the
fixture's key lists, the refusals that need no GPU, and the guard that the fixture's masks are decidable at the GPU tests' band.

Measured: the restatement with ``table="as_reference"`` differs from F24 by at most 4.3e-14 on pred_masks of magnitude 58 and by at most
3.8e-15 on every other output (the bound asserted below is 64 ulp of fp64 at the output's magnitude), and reproduces every stored
attention mask bit for bit.  The share of mask bits whose fp64 logit lies inside the band (4 x the operand-precision floor of the layer's
logits) is 0 in fp32 mode and at most 2.1 % in bf16 mode (case cl_wrap, layer 3), under half of the GPU tests' cap of 5 %.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mask_decoder_oracle as DO
from tests.helpers import EPS32, MARGIN, maxabs

MODES = {"fp32": "x3", "bf16": True}
CAP = 0.05


def _module(c, **kw):
    import streamformer_amd as sa
    return getattr(sa, c["cls"])(c["in_channels"], **dict(DO.decoder_kwargs(c), **kw))


@pytest.fixture(scope="module")
def golden():
    return DO.load_golden()


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c)
    return DO.forward(DO.make_weights(c), c, xs, mf, table="as_reference")


@pytest.mark.parametrize("name", list(DO.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    c = DO.CASES[name]
    assert int(golden[f"{name}.seed"]) == c["seed"]
    xs, mf = DO.make_inputs(c)
    for k, v in [(f"x{l}", x) for l, x in enumerate(xs)] + [("mask_features", mf)]:
        assert torch.equal(torch.from_numpy(golden[f"{name}.{k}"].astype("float32")), v)
    got = _reference(name)
    keys = [k for k in DO.OUTPUTS if f"{name}.{k}" in golden]
    assert keys == list(DO.OUTPUTS if DO.is_cl(c) else DO.OUTPUTS[:2])
    for k in keys:
        want = torch.from_numpy(golden[f"{name}.{k}"])
        assert got[k].shape == want.shape
        gap = maxabs(got[k], want)
        print(f"  {name}.{k}: gap {gap:.3e}")
        assert gap <= 64 * 2.0 ** -53 * float(want.abs().max())
    for i, m in enumerate(got["attn_masks"]):
        assert np.array_equal(DO.pack_mask(m.numpy()), golden[f"{name}.attn_mask{i}"]), (name, i)
        assert np.array_equal(DO.unpack_mask(golden[f"{name}.attn_mask{i}"], m.shape[-1]), m.numpy())


def test_fixture_takes_the_all_masked_rule_and_hides_whole_tiles():
    """Asserted on the oracle's masks: rows whose threshold is set everywhere (cleared by the reference's rule), and a 16-key tile hidden
    from all queries of an aligned 16-query tile: what the attention kernel skips."""
    cleared = tiles = 0
    for name in DO.CASES:
        got = _reference(name)
        for low, m in zip(got["low_logits"], got["attn_masks"]):
            raw = low < 0
            full = raw.all(-1)
            cleared += int(full.sum())
            assert not m[full].any() and torch.equal(m[~full], raw[~full])
            Q, P = m.shape[1:]
            for q0 in range(0, Q, 16):
                for k0 in range(0, P - 15, 16):
                    tiles += int(m[:, q0:q0 + 16, k0:k0 + 16].all(-1).all(-1).sum())
    print(f"  rows cleared {cleared}, hidden 16 x 16 tiles {tiles}")
    assert cleared > 0 and tiles > 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(DO.CASES))
def test_undecided_share_stays_under_half_the_cap(name, mode):
    """The band of the GPU tests is 4 x the operand-precision floor of a layer's logits; the share of the reference's own mask bits inside
    it must leave the GPU tests' cap (5 % of a layer's bits) a factor of two."""
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c)
    sd = DO.make_weights(c)
    want = DO.forward(sd, c, xs, mf, table="fp64")
    floor = DO.forward(sd, c, xs, mf, dtype=torch.float32, operands=MODES[mode], table="fp64", masks=want["attn_masks"], interp="features")
    for i, (w, f) in enumerate(zip(want["low_logits"], floor["low_logits"])):
        band = MARGIN * max(maxabs(f, w), EPS32 * float(w.abs().max()))
        share = float((w.abs() <= band).double().mean())
        print(f"  {name} {mode} layer {i}: band {band:.3e}, undecided share {share:.4f}")
        assert share <= CAP / 2, (name, mode, i, share)


@pytest.mark.parametrize("name", list(DO.CASES))
def test_module_parameter_tree_is_the_references(golden, name):
    c = DO.CASES[name]
    m = _module(c)
    sd = m.state_dict()
    assert list(sd) == list(golden[f"{name}.keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(golden[f"{name}.shapes"])
    assert list(DO.key_kinds(c)) == list(sd)
    w = DO.make_weights(c)
    res = m.load_state_dict(w, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(m.state_dict()[k], v) for k, v in w.items())
    # the checkpoint's prefix is accepted and dropped
    m2 = _module(c)
    m2.load_state_dict({"sem_seg_head.predictor." + k: v for k, v in w.items()}, strict=True)
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in w.items())
    # an old checkpoint's static_query becomes query_feat
    m3 = _module(c)
    old = {("sem_seg_head.predictor." + k).replace("query_feat", "static_query"): v for k, v in w.items()}
    assert any("static_query" in k for k in old)
    m3.load_state_dict(old, strict=True)
    assert all(torch.equal(m3.state_dict()[k], v) for k, v in w.items())
    assert isinstance(m.input_proj[0], torch.nn.Sequential) == (not DO.has_proj(c))


def test_initialisation_is_the_references():
    torch.manual_seed(0)
    c = DO.CASES["cl"]
    m = _module(c)
    C_ = c["hidden"]
    bound = lambda fan_in, fan_out: (6.0 / (fan_in + fan_out)) ** 0.5      # noqa: E731
    w = m.transformer_cross_attention_layers[0].multihead_attn.in_proj_weight.detach()
    assert float(w.abs().max()) <= bound(C_, 3 * C_) and float(w.abs().max()) > 0.9 * bound(C_, 3 * C_)
    w = m.transformer_ffn_layers[0].linear1.weight.detach()
    assert float(w.abs().max()) <= bound(C_, c["ffn"])
    for conv in list(m.input_proj) + list(m.reid_embed.layers):          # c2_xavier_fill: uniform(+-sqrt(3 / fan_in)), zero bias
        fan_in = conv.weight[0].numel()
        assert float(conv.weight.detach().abs().max()) <= (3.0 / fan_in) ** 0.5 and not conv.bias.any()


def test_constructor_refusals_name_the_argument():
    c = DO.CASES["cl"]
    with pytest.raises(NotImplementedError, match="pre_norm"):
        _module(c, pre_norm=True)
    with pytest.raises(NotImplementedError, match="mask_classification"):
        _module(c, mask_classification=False)
    for field in ("hidden_dim", "dim_feedforward", "mask_dim", "reid_hidden_dim"):
        with pytest.raises(ValueError, match=field):
            _module(c, **{field: 96})
    with pytest.raises(ValueError, match="in_channels"):
        import streamformer_amd as sa
        sa.CLMultiScaleMaskedTransformerDecoder(96, **DO.decoder_kwargs(c))
    with pytest.raises(ValueError, match="nheads"):
        _module(c, nheads=32)                # 128 / 32 = 4 channels per head
    with pytest.raises(ValueError, match="compute_dtype"):
        _module(c, compute_dtype="fp16")


def test_forward_refusals_without_a_gpu():
    c = DO.CASES["cl"]
    m = _module(c)
    xs, mf = DO.make_inputs(c)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(xs, mf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(xs, mf)


def _config(**kw):
    import streamformer_amd._native as nat
    base = dict(in_channels=64, hidden_dim=128, num_queries=5, nheads=4, dim_feedforward=128, dec_layers=1, mask_dim=64, num_classes=3,
                enforce_input_project=0, pre_norm=0, mask_classification=1, reid_layers=3, reid_hidden_dim=64)
    base.update(kw)
    return nat.SfMaskdecConfig(*[base[n] for n, _ in nat.SfMaskdecConfig._fields_])


@pytest.mark.parametrize("field,kw", [
    ("pre_norm", dict(pre_norm=1)),
    ("mask_classification", dict(mask_classification=0)),
    ("hidden_dim", dict(hidden_dim=96)),
    ("hidden_dim", dict(hidden_dim=0)),
    ("dim_feedforward", dict(dim_feedforward=100)),
    ("mask_dim", dict(mask_dim=32)),
    ("in_channels", dict(in_channels=72)),
    ("reid_hidden_dim", dict(reid_hidden_dim=48)),
    ("hidden_dim / nheads", dict(nheads=32)),
    ("hidden_dim / nheads", dict(hidden_dim=256, nheads=1)),
    ("num_queries", dict(num_queries=0)),
    ("num_classes", dict(num_classes=0)),
    ("dec_layers", dict(dec_layers=65)),
    ("reid_layers", dict(reid_layers=-2)),
])
def test_handle_refuses_by_field(field, kw):
    import streamformer_amd._native as nat
    h = C.c_void_p()
    cfg = _config(**kw)
    assert nat.lib.sf_maskdec_create(C.byref(cfg), 0, C.byref(h)) == nat.SF_ERR_INVALID
    assert field.encode() in nat.lib.sf_last_error(), nat.lib.sf_last_error()
    assert not h.value


def test_handle_keys_and_state_without_a_gpu():
    import streamformer_amd._native as nat
    h = C.c_void_p()
    cfg = _config()
    assert nat.lib.sf_maskdec_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        n_keys = len(DO.key_kinds(DO.CASES["cl"]))
        assert nat.lib.sf_maskdec_missing_weights(h) == n_keys and b"missing" in nat.lib.sf_last_error()
        w = np.zeros((5, 128), np.float32)
        shape = (C.c_int64 * 2)(*w.shape)
        for key in (b"query_feat.weight", b"sem_seg_head.predictor.query_embed.weight"):
            assert nat.lib.sf_maskdec_load_tensor(h, key, w.ctypes.data, nat.SF_F32, shape, 2) == 0
        assert nat.lib.sf_maskdec_load_tensor(h, b"static_query.weight", w.ctypes.data, nat.SF_F32, shape, 2) == nat.SF_ERR_UNKNOWN_KEY
        assert nat.lib.sf_maskdec_load_tensor(h, b"query_feat.weight", w.ctypes.data, nat.SF_F16, shape, 2) == nat.SF_ERR_INVALID
        bad = (C.c_int64 * 2)(128, 5)
        assert nat.lib.sf_maskdec_load_tensor(h, b"query_feat.weight", w.ctypes.data, nat.SF_F32, bad, 2) == nat.SF_ERR_INVALID
        assert nat.lib.sf_maskdec_missing_weights(h) == n_keys - 2
        shapes = (C.c_int32 * 6)(2, 3, 4, 6, 7, 9)
        nbytes = C.c_size_t()
        assert nat.lib.sf_maskdec_workspace_bytes(h, 2, shapes, 8, 12, C.byref(nbytes)) == nat.SF_ERR_STATE
        assert nat.lib.sf_maskdec_workspace_bytes(h, 0, shapes, 8, 12, C.byref(nbytes)) == nat.SF_ERR_INVALID and b"frames" in nat.lib.sf_last_error()
    finally:
        nat.lib.sf_maskdec_destroy(h)
