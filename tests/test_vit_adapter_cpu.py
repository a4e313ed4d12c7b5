"""ViT-Adapter without a GPU: the fp64 restatement (tests/vit_adapter_oracle.py) against fixture F22, which the reference's own class wrote;
the module's parameter tree, state-dict round trip and every refusal."""
import copy

import numpy as np
import pytest
import torch

from oracle import streamformer_oracle as O
from tests import vit_adapter_oracle as VO
from tests.oracle_ops import operand_linear

REL = 1e-10


@pytest.fixture(scope="module")
def golden():
    return VO.load_golden()


def _adapter(c, **over):
    import streamformer_amd as sa
    kw = VO.adapter_kwargs(c)
    cfg = over.pop("config", None) or VO.config(c)
    kw.update(over)
    return sa.TimesformerMultiTaskingModelSigLIPViTAdapter(cfg, **kw)


@pytest.mark.parametrize("name", list(VO.CASES))
def test_fp64_restatement_reproduces_f22(golden, name):
    c = VO.CASES[name]
    assert int(golden[f"{name}.seed"]) == c["seed"]
    pixels = torch.from_numpy(golden[f"{name}.pixels"].astype(np.float32))
    assert torch.equal(pixels, VO.make_pixels(c))
    res, cs = VO.forward(VO.make_weights(c), c, pixels)
    assert list(res) == list(VO.OUTPUTS) and len(cs) == len(c["indexes"])
    Hg, Wg = VO.grid(c)
    for k, (h, w) in zip(VO.OUTPUTS, ((4 * Hg, 4 * Wg), (2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2))):
        want = torch.from_numpy(golden[f"{name}.{k}"])
        assert tuple(want.shape) == (c["B"] * c["T"], c["hidden"], h, w) and want.dtype == torch.float64
        assert float((res[k] - want).abs().max()) <= REL * float(want.abs().max()), k
    for i, got in enumerate(cs):
        want = torch.from_numpy(golden[f"{name}.c{i}"])
        assert float((got - want).abs().max()) <= REL * float(want.abs().max()), i


def test_encoder_layer_restatement_equals_the_encoder_oracle():
    """encoder_layer (the oracle's layer with the Linear and the operand rounding as arguments) in fp64 is oracle.layer_forward."""
    c = VO.CASES["sq"]
    cfg = VO.config(c)
    sd = O.cast_state_dict(VO.make_weights(c), torch.float64)
    h = torch.from_numpy(np.random.RandomState(5).standard_normal((2, 2, 16, c["hidden"])))
    lin = lambda x, w, b: operand_linear(x, w, b, False)      # noqa: E731
    for i in range(2):
        want = O.layer_forward(sd, cfg, i, h)
        assert float((VO.encoder_layer(sd, cfg, i, h, lin, lambda t: t) - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name", list(VO.CASES))
def test_module_has_the_reference_tree(golden, name):
    c = VO.CASES[name]
    m = _adapter(c)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in golden[f"{name}.keys"]], "keys or their order differ from the reference's state dict"
    want = VO.make_weights(c)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert not any(k.startswith("head.") for k in sd)
    assert sd["norm1.num_batches_tracked"].dtype == torch.int64 and not m.training
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert frozen and all(k.split(".")[0] in ("embeddings", "encoder", "post_layernorm") for k in frozen)
    assert all(p.requires_grad for k, p in m.named_parameters() if k.split(".")[0] not in ("embeddings", "encoder", "post_layernorm"))


def test_initialisation_rules():
    c = VO.CASES["sq"]
    torch.manual_seed(0)
    m = _adapter(c).requires_grad_(False)
    ex = m.interactions[3].extra_extractors[1]
    D = c["hidden"]
    for lin in (ex.attn.sampling_offsets, ex.attn.attention_weights, ex.attn.value_proj, ex.attn.output_proj, ex.ffn.fc1, ex.ffn.fc2):
        assert float(lin.bias.abs().max()) == 0.0 and float(lin.weight.abs().max()) <= 2.0 and 0.015 < float(lin.weight.std()) < 0.025
    for conv, fan_out in ((m.spm.stem[0], 9 * 64), (m.spm.fc3, D), (m.up, 4 * D), (ex.ffn.dwconv.dwconv, 9)):
        assert 0.8 < float(conv.weight.std()) / (2.0 / fan_out) ** 0.5 < 1.2
        assert conv.bias is None or float(conv.bias.abs().max()) == 0.0
    assert 0.8 < float(m.level_embed.std()) < 1.2
    assert torch.equal(m.norm2.running_var, torch.ones(D)) and torch.equal(ex.ffn_norm.weight, torch.ones(D))


def test_state_dict_round_trip_and_copy():
    c = VO.CASES["sq"]
    sd = VO.make_weights(c)
    m = _adapter(c)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(sd) or set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    m2 = copy.deepcopy(m)
    assert all(torch.equal(v, back[k]) for k, v in m2.state_dict().items())
    assert m2.embeddings is m2._enc.embeddings and m2._enc is not m._enc
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "up.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{"head.probe": torch.zeros(1, 1, c["hidden"])}), strict=True)


def test_refusals_name_the_field():
    import streamformer_amd as sa
    c = VO.CASES["sq"]
    base = VO.config(c).to_dict()

    def cfg(**kw):
        return sa.StreamformerConfig(**dict(base, **kw))

    with pytest.raises(NotImplementedError, match="patch_size"):
        _adapter(c, config=cfg(patch_size=8))
    with pytest.raises(NotImplementedError, match="with_cp"):
        _adapter(c, with_cp=True)
    with pytest.raises(ValueError, match="hidden_size"):
        _adapter(c, config=cfg(hidden_size=96))
    with pytest.raises(ValueError, match="cffn_ratio"):
        _adapter(c, cffn_ratio=0.25)                       # 128 * 0.25 = 32
    for heads in (3, 32):                                  # 128 / 3 is no whole width; 128 / 32 = 4 is below the kernel's 8
        with pytest.raises(ValueError, match="deform_num_heads"):
            _adapter(c, deform_num_heads=heads)
    for bad in ([[0, 1], [3, 3]], [[0, 1], [2, 2]], [[1, 3]], [[0, 0], [1, 1], [2, 2], [3, 4]], [[0, 3], [2, 3]]):
        with pytest.raises(ValueError, match="interaction_indexes"):
            _adapter(c, interaction_indexes=bad, add_vit_feature=False)
    with pytest.raises(ValueError, match="interaction_indexes"):
        _adapter(c, interaction_indexes=[[0, 1], [2, 3]])  # add_vit_feature adds the maps of exactly four blocks
    m = _adapter(c)
    for H, W, field in ((48, 64, "H"), (64, 80, "W")):
        with pytest.raises(ValueError, match=field):
            m(torch.zeros(1, 1, 3, H, W))
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()(torch.zeros(1, 1, 3, 64, 64))
    m.eval()
    with pytest.raises(RuntimeError, match="runs on the MI355X"):
        m(VO.make_pixels(c))
