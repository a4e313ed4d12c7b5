"""CPU: the connector's oracle against the reference's own outputs (tests/golden/f19_connector.npz), the parameter tree and its
checkpoint round trip, the token count, and every refusal that needs no GPU."""
import ctypes as C
import itertools

import pytest
import torch

from tests import connector_oracle as CO
from tests.helpers import MARGIN, fp32_floor, maxabs


@pytest.fixture(scope="module")
def gold():
    return CO.load_golden()


@pytest.mark.parametrize("name", list(CO.CASES))
def test_oracle_reproduces_the_reference(gold, name):
    sd, cfg, feats, ref = CO.golden_case(gold, name)
    # the stored weights are the ones the seeds redraw
    redrawn = CO.make_weights(cfg["mm_projector_type"], int(gold[f"w.{cfg['mm_projector_type']}.seed"]))
    assert set(redrawn) == set(sd) and all(torch.equal(redrawn[k], sd[k]) for k in redrawn)
    want = CO.forward(sd, cfg, feats)
    floor = fp32_floor(CO.forward(sd, cfg, feats, dtype=torch.float32), want)
    assert ref.shape == want.shape == (CO.num_tokens(cfg, CO.FRAMES, CO.CASES[name][2]), CO.D_OUT)
    err = maxabs(ref, want)
    print(f"[connector oracle {name}] reference fp32 vs fp64 restatement {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}")
    assert err <= MARGIN * floor
    # the newline rows are the parameter itself
    if CO.CASES[name][3] == "grid":
        Po = CO.pooled_side(CO.CASES[name][2], cfg["mm_spatial_pool_mode"], 2)
        assert torch.equal(ref[Po], sd["image_newline"]) and torch.equal(ref[-1], sd["image_newline"])
    elif CO.CASES[name][3] in ("frame", "one_token"):
        assert torch.equal(ref[-1], sd["image_newline"])


def test_stride_two_bilinear_on_an_even_grid_is_the_two_by_two_average():
    """The oracle's taps (the sentence in DESIGN.md 3.9), and the package's cell count for the same grids: equal on an even grid,
    ceil against floor on an odd one."""
    import streamformer_amd as sa
    from streamformer_amd.connector import pooled_side
    bil, avg = (sa.VideoTokenConnector(CO.make_config("linear", mode, "grid", stride=2)) for mode in ("bilinear", "average"))
    for P in (2, 6, 14):
        assert torch.equal(CO.tap_matrix(P, "bilinear", 2), CO.tap_matrix(P, "average", 2))
        assert pooled_side(P, "bilinear", 2) == pooled_side(P, "average", 2) == P // 2
        assert bil.num_tokens(3, P) == avg.num_tokens(3, P) == 3 * (P // 2) * (P // 2 + 1)
    assert not torch.equal(CO.tap_matrix(5, "bilinear", 2)[:2], CO.tap_matrix(5, "average", 2))
    assert (pooled_side(5, "bilinear", 2), pooled_side(5, "average", 2)) == (3, 2)
    assert (bil.num_tokens(3, 5), avg.num_tokens(3, 5)) == (3 * 3 * 4, 3 * 2 * 3)


@pytest.mark.parametrize("proj", ["mlp2x_gelu", "linear"])
def test_parameter_keys_and_checkpoint_round_trip(gold, tmp_path, proj):
    import streamformer_amd as sa
    sd = CO.golden_weights(gold, proj)
    cfg = CO.make_config(proj, "bilinear", "grid")
    m = sa.VideoTokenConnector(cfg)
    assert set(m.state_dict()) == set(sd)                       # the reference builder's names (the generator loaded them strictly)
    assert all(not p.requires_grad for p in m.parameters())
    m.load_state_dict({"model." + k: v for k, v in sd.items()})
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{"model.layers.0.mlp.up_proj.weight": torch.zeros(2)}))
    r = m.load_state_dict(dict(sd, **{"model.layers.0.mlp.up_proj.weight": torch.zeros(2)}), strict=False)
    assert not r.missing_keys and not r.unexpected_keys
    m.save_pretrained(str(tmp_path))
    saved = torch.load(str(tmp_path / "mm_projector.bin"), weights_only=True)
    assert set(saved) == {"model." + k for k in sd}             # LLaVA's adapter file
    m2 = sa.VideoTokenConnector.from_pretrained(str(tmp_path), device="cpu")
    assert m2.config == m.config and all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    # no newline parameter without "unpad" and without newline rows (llava_arch:45)
    flat = sa.VideoTokenConnector(CO.make_config(proj, merge="flat"))
    assert "image_newline" not in flat.state_dict() and flat.newline == "no_token"
    assert sa.VideoTokenConnector(CO.make_config(proj, newline="one_token", merge="spatial")).newline == "no_token"


def test_defaults_follow_the_reference():
    import streamformer_amd as sa
    m = sa.VideoTokenConnector({"mm_hidden_size": 64, "hidden_size": 128, "mm_patch_merge_type": "spatial_unpad"})
    assert (m.projector_type, m.pool_mode, m.pool_stride, m.newline) == ("linear", "bilinear", 2, "one_token")
    assert list(m.state_dict()) == ["image_newline", "mm_projector.weight", "mm_projector.bias"]

    class Cfg:
        mm_projector_type = "mlp2x_gelu"
        mm_hidden_size = 64
        hidden_size = 128
        mm_spatial_pool_stride = None
    assert sa.VideoTokenConnector(Cfg()).num_tokens(2, 14) == 2 * 49          # flat: no newline rows


@pytest.mark.parametrize("mode", ["average", "max", "bilinear"])
def test_num_tokens_equals_the_oracle_length(mode):
    import streamformer_amd as sa
    import streamformer_amd._native as nat
    F = 3
    for P, stride, newline in itertools.product((2, 3, 5, 6, 9, 14), (1, 2, 4), ("no_token", "one_token", "frame", "grid")):
        cfg = CO.make_config("linear", mode, newline, stride=stride)
        m = sa.VideoTokenConnector(cfg)
        if CO.pooled_side(P, mode, stride) < 1:
            with pytest.raises(nat.NativeError) as e:
                m.num_tokens(F, P)
            assert e.value.code == nat.SF_ERR_INVALID
            continue
        sd = CO.make_weights("linear", 7)
        want = CO.forward(sd, cfg, CO.make_features(3, F, P), dtype=torch.float32)
        assert m.num_tokens(F, P) == want.shape[0] == CO.num_tokens(cfg, F, P), (P, stride, newline)


def test_python_refusals():
    import streamformer_amd as sa
    base = CO.make_config()
    with pytest.raises(NotImplementedError, match="add_faster_video"):
        sa.VideoTokenConnector(dict(base, add_faster_video=True))
    for t in ("pooler", "mlp2x_res2x_gelu"):
        with pytest.raises(NotImplementedError, match="mm_projector_type"):
            sa.VideoTokenConnector(dict(base, mm_projector_type=t))
    with pytest.raises(ValueError, match="Unknown projector type"):
        sa.VideoTokenConnector(dict(base, mm_projector_type="qformer"))
    with pytest.raises(ValueError, match="mm_spatial_pool_mode"):
        sa.VideoTokenConnector(dict(base, mm_spatial_pool_mode="median"))
    with pytest.raises(ValueError, match="mm_newline_position"):
        sa.VideoTokenConnector(dict(base, mm_newline_position="column"))
    m = sa.VideoTokenConnector(dict(base, image_aspect_ratio="anyres_max_9"))
    with pytest.raises(NotImplementedError, match="image_aspect_ratio"):
        m(torch.zeros(2, 25, CO.D_IN), modality="image")
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(2, 24, CO.D_IN))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 25, CO.D_IN + 8))


def _create(nat, *fields):
    h = C.c_void_p()
    rc = nat.lib.sf_connector_create(C.byref(nat.SfConnectorConfig(*fields)), 0, C.byref(h))
    return rc, h


def test_native_refusals_and_load_tensor():
    import streamformer_amd._native as nat
    for bad in ((72, 128, 2, 3, 2, 3), (64, 100, 2, 3, 2, 3), (64, 128, -1, 3, 2, 3), (64, 128, 0, 3, 2, 3), (64, 128, 2, 4, 2, 3),
                (64, 128, 2, 3, 0, 3), (64, 128, 2, 3, 2, 4)):
        rc, _ = _create(nat, *bad)
        assert rc == nat.SF_ERR_INVALID and nat.lib.sf_last_error(), bad
    rc, h = _create(nat, 64, 128, 2, 3, 2, 3)
    assert rc == 0
    try:
        n = C.c_int64()
        assert nat.lib.sf_connector_num_tokens(h, 2, 5, C.byref(n)) == 0 and n.value == 2 * 3 * 4
        assert nat.lib.sf_connector_num_tokens(h, 2, 0, C.byref(n)) == nat.SF_ERR_INVALID           # P < 1
        assert nat.lib.sf_connector_num_tokens(h, 0, 5, C.byref(n)) == nat.SF_ERR_INVALID
        # 2^31 - 1 elements per activation: 16 frames x 1024^2 patches x 128 columns
        assert nat.lib.sf_connector_num_tokens(h, 16, 1024, C.byref(n)) == nat.SF_ERR_CAPACITY and b"2^31" in nat.lib.sf_last_error()
        sz = C.c_size_t()
        assert nat.lib.sf_connector_workspace_bytes(h, 2, 5, C.byref(sz)) == nat.SF_ERR_STATE      # not finalized
        assert nat.lib.sf_connector_forward(h, 256, 2, 0, 256, nat.SF_F32, 256, 1 << 20, None) == nat.SF_ERR_INVALID
        assert nat.lib.sf_connector_forward(h, 256, 2, 5, 256, nat.SF_F32, 256, 1 << 20, None) == nat.SF_ERR_STATE

        def load(key, t):
            shape = (C.c_int64 * t.dim())(*t.shape)
            return nat.lib.sf_connector_load_tensor(h, key.encode(), t.data_ptr(), nat.SF_F32, shape, t.dim())
        assert load("model.vision_tower.embeddings.weight", torch.zeros(4)) == nat.SF_ERR_UNKNOWN_KEY
        assert load("mm_projector.weight", torch.zeros(128, 64)) == nat.SF_ERR_UNKNOWN_KEY          # the "linear" name on an mlp2x projector
        assert load("mm_projector.1.weight", torch.zeros(128, 64)) == nat.SF_ERR_UNKNOWN_KEY        # the GELU's index
        assert load("mm_projector.0.weight", torch.zeros(64, 128)) == nat.SF_ERR_INVALID            # transposed
        assert load("mm_projector.2.weight", torch.zeros(128, 64)) == nat.SF_ERR_INVALID
        assert load("image_newline", torch.zeros(64)) == nat.SF_ERR_INVALID
        assert nat.lib.sf_connector_missing_weights(h) == 5 and b"image_newline" in nat.lib.sf_last_error()
        assert load("mm_projector.0.weight", torch.zeros(128, 64)) == 0
        assert load("model.mm_projector.0.bias", torch.zeros(128)) == 0
        assert load("model.mm_projector.2.weight", torch.zeros(128, 128)) == 0
        assert load("mm_projector.2.bias", torch.zeros(128)) == 0
        assert nat.lib.sf_connector_missing_weights(h) == 1                                       # image_newline: newline = grid
        assert load("model.image_newline", torch.zeros(128)) == 0
        assert nat.lib.sf_connector_missing_weights(h) == 0
    finally:
        nat.lib.sf_connector_destroy(h)
    rc, h = _create(nat, 64, 128, 1, 3, 2, 0)
    assert rc == 0
    assert nat.lib.sf_connector_missing_weights(h) == 2                                            # no newline rows: image_newline not required
    nat.lib.sf_connector_destroy(h)
    # the kernel's own argument checks, before any launch
    for args in ((256, None, None, 1, 0, 64, 3, 2, 0, None, 256, nat.SF_F32, None, None),          # P = 0
                 (256, None, None, 1, 2, 64, 1, 4, 0, None, 256, nat.SF_F32, None, None),          # 2 x 2 averaged with stride 4: no cell
                 (256, None, None, 1, 5, 60, 3, 2, 0, None, 256, nat.SF_F32, None, None),          # C % 8
                 (256, None, None, 1, 5, 64, 3, 2, 3, None, 256, nat.SF_F32, None, None),          # grid without newline_dev
                 (264, None, None, 1, 5, 64, 3, 2, 0, None, 256, nat.SF_F32, None, None),          # 8-byte aligned input
                 (256, 256, None, 1, 5, 64, 3, 2, 0, None, 256, nat.SF_F32, None, None),           # both input forms
                 (None, 256, None, 1, 5, 64, 3, 2, 0, None, 256, nat.SF_F32, None, None)):         # planes in, fp32 out
        assert nat.lib.sf_op_connector_pool(*args, None) == nat.SF_ERR_INVALID, args
    assert nat.lib.sf_op_connector_pool(256, None, None, 4096, 64, 128, 3, 2, 0, None, 256, nat.SF_F32, None, None, None) == nat.SF_ERR_CAPACITY
