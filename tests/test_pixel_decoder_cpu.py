"""CPU: the pixel decoder's fp64 restatement against fixture F23 (the reference's own class), the module's parameter tree against the
fixture's key list, and the refusals that need no GPU.

Measured: the restatement with ``table="as_reference"`` differs from F23 by at most 3.8e-15 (fp64 rounding of values up to 4); the fp64
position table moves the result by 1.4e-7, which is why the GPU tests take their ``want`` from ``table="fp64"``.
"""
import ctypes as C

import pytest
import torch

from tests import pixel_decoder_oracle as PO
from tests.helpers import maxabs


def _module(c, **kw):
    import streamformer_amd as sa
    shape = {k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, c["channels"], PO.STRIDES)}
    return sa.MSDeformAttnPixelDecoder(shape, **dict(PO.decoder_kwargs(c), **kw))


@pytest.fixture(scope="module")
def golden():
    return PO.load_golden()


@pytest.mark.parametrize("name", list(PO.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    c = PO.CASES[name]
    assert int(golden[f"{name}.seed"]) == c["seed"]
    feats = PO.make_features(c)
    for k, v in feats.items():
        assert torch.equal(torch.from_numpy(golden[f"{name}.{k}"].astype("float32")), v)
    locs = []
    mask, out = PO.forward(PO.make_weights(c), c, feats, table="as_reference", locations=locs)
    pairs = [("mask_features", mask)] + [(f"out{i}", o) for i, o in enumerate(out[:3])]
    for key, got in pairs:
        want = torch.from_numpy(golden[f"{name}.{key}"])
        assert got.shape == want.shape
        gap = maxabs(got, want)
        print(f"  {name}.{key}: gap {gap:.3e}")
        assert gap <= 64 * 2.0 ** -53 * float(want.abs().max())
    # the weight draw makes the sampling depend on the query and leave the unit square (samples cross their level's border)
    for loc in locs:
        outside = ((loc < 0) | (loc > 1)).double().mean()
        assert 0.05 < float(outside) < 0.95 and float(loc.std(1).min()) > 0


@pytest.mark.parametrize("name", list(PO.CASES))
def test_module_parameter_tree_is_the_references(golden, name):
    c = PO.CASES[name]
    m = _module(c)
    sd = m.state_dict()
    assert list(sd) == list(golden[f"{name}.keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(golden[f"{name}.shapes"])
    assert list(PO.key_kinds(c)) == list(sd)
    w = PO.make_weights(c)
    res = m.load_state_dict(w, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(m.state_dict()[k], v) for k, v in w.items())
    # the checkpoint's prefix is accepted and dropped
    m2 = _module(c)
    m2.load_state_dict({"sem_seg_head.pixel_decoder." + k: v for k, v in w.items()}, strict=True)
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in w.items())
    assert m.num_fpn_levels == PO.num_fpn(c)


def test_constructor_refusals_name_the_argument():
    import streamformer_amd as sa
    c = PO.CASES["m2f"]
    shape = lambda ch: {k: sa.ShapeSpec(v, s) for k, v, s in zip(PO.LEVELS, ch, PO.STRIDES)}      # noqa: E731
    kw = PO.decoder_kwargs(c)
    with pytest.raises(NotImplementedError, match="norm"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, norm="SyncBN"))
    with pytest.raises(NotImplementedError, match="norm"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, norm=""))
    with pytest.raises(ValueError, match="channels"):
        sa.MSDeformAttnPixelDecoder(shape((64, 128, 96, 192)), **kw)
    with pytest.raises(ValueError, match="conv_dim"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, conv_dim=96))
    with pytest.raises(ValueError, match="transformer_dim_feedforward"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, transformer_dim_feedforward=100))
    with pytest.raises(ValueError, match="transformer_nheads"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, transformer_nheads=16))          # 64 / 16 = 4 channels per head
    with pytest.raises(ValueError, match="compute_dtype"):
        sa.MSDeformAttnPixelDecoder(shape(c["channels"]), **dict(kw, compute_dtype="fp16"))


def test_forward_refusals_without_a_gpu():
    c = PO.CASES["m2f"]
    m = _module(c)
    feats = PO.make_features(c)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train().forward_features(feats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval().forward_features(feats)


def _config(**kw):
    import streamformer_amd._native as nat
    base = dict(num_levels=4, channels=(64, 128, 64, 192), strides=(4, 8, 16, 32), in_transformer=(0, 1, 1, 1), conv_dim=64, mask_dim=64, nheads=8,
                dim_feedforward=128, enc_layers=2, enc_n_points=4, common_stride=4, norm=0, im2col_chunk_rows=0)
    base.update(kw)
    arr = lambda v: (C.c_int32 * 4)(*v)      # noqa: E731
    return nat.SfPixdecConfig(base["num_levels"], arr(base["channels"]), arr(base["strides"]), arr(base["in_transformer"]), base["conv_dim"],
                              base["mask_dim"], base["nheads"], base["dim_feedforward"], base["enc_layers"], base["enc_n_points"],
                              base["common_stride"], base["norm"], base["im2col_chunk_rows"])


@pytest.mark.parametrize("field,kw", [
    ("channels[2]", dict(channels=(64, 128, 96, 192))),
    ("conv_dim", dict(conv_dim=96)),
    ("conv_dim", dict(conv_dim=0)),
    ("dim_feedforward", dict(dim_feedforward=100)),
    ("conv_dim / nheads", dict(nheads=16)),
    ("conv_dim / nheads", dict(conv_dim=256, nheads=1)),
    ("enc_n_points", dict(enc_n_points=9)),
    ("norm", dict(norm=1)),
    ("num_levels", dict(num_levels=5)),
    ("in_transformer", dict(in_transformer=(0, 0, 0, 0))),
    ("common_stride", dict(common_stride=1)),
    ("im2col_chunk_rows", dict(im2col_chunk_rows=-1)),
])
def test_handle_refuses_by_field(field, kw):
    import streamformer_amd._native as nat
    h = C.c_void_p()
    cfg = _config(**kw)
    assert nat.lib.sf_pixdec_create(C.byref(cfg), 0, C.byref(h)) == nat.SF_ERR_INVALID
    assert field.encode() in nat.lib.sf_last_error(), nat.lib.sf_last_error()
    assert not h.value


def test_handle_keys_and_state_without_a_gpu():
    import numpy as np
    import streamformer_amd._native as nat
    h = C.c_void_p()
    cfg = _config()
    assert nat.lib.sf_pixdec_create(C.byref(cfg), 0, C.byref(h)) == 0
    try:
        n_keys = len(PO.key_kinds(PO.CASES["m2f"]))
        assert nat.lib.sf_pixdec_missing_weights(h) == n_keys and b"missing" in nat.lib.sf_last_error()
        n_ms, n_fpn = C.c_int(), C.c_int()
        assert nat.lib.sf_pixdec_num_outputs(h, C.byref(n_ms), C.byref(n_fpn)) == 0 and (n_ms.value, n_fpn.value) == (3, 1)
        w = np.zeros((64, 64, 3, 3), np.float32)
        shape = (C.c_int64 * 4)(*w.shape)
        for key in (b"layer_1.weight", b"sem_seg_head.pixel_decoder.layer_1.weight"):
            assert nat.lib.sf_pixdec_load_tensor(h, key, w.ctypes.data, nat.SF_F32, shape, 4) == 0
        assert nat.lib.sf_pixdec_load_tensor(h, b"layer_2.weight", w.ctypes.data, nat.SF_F32, shape, 4) == nat.SF_ERR_UNKNOWN_KEY
        assert nat.lib.sf_pixdec_load_tensor(h, b"layer_1.weight", w.ctypes.data, nat.SF_F16, shape, 4) == nat.SF_ERR_INVALID
        bad = (C.c_int64 * 2)(64, 576)
        assert nat.lib.sf_pixdec_load_tensor(h, b"layer_1.weight", w.ctypes.data, nat.SF_F32, bad, 2) == nat.SF_ERR_INVALID
        assert nat.lib.sf_pixdec_missing_weights(h) == n_keys - 1
        shapes = (C.c_int32 * 8)(12, 20, 6, 10, 3, 5, 2, 3)
        nbytes = C.c_size_t()
        assert nat.lib.sf_pixdec_workspace_bytes(h, 2, shapes, 4, C.byref(nbytes)) == nat.SF_ERR_STATE
        assert nat.lib.sf_pixdec_workspace_bytes(h, 2, shapes, 3, C.byref(nbytes)) == nat.SF_ERR_INVALID and b"level" in nat.lib.sf_last_error()
    finally:
        nat.lib.sf_pixdec_destroy(h)
