"""CPU side of the native SigLIP text tower: the fp64 restatement the GPU tests measure against reproduces the HF fixture, the
module carries HF's parameter tree, checkpoints round-trip, the wrapper without a tower is what it was, and every refusal comes with
a message before anything reaches the GPU (these tests run on a machine without one)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import text_tower_oracle as TO

# HF computes in fp32, the restatement in fp64: what separates them is fp32 rounding through sums of up to 1072 products of O(1)
# terms — about sqrt(K) * 2^-24 * |x| = 33 * 6e-8 * 4 = 8e-6 per Linear, a few Linears deep.  (2.4e-6 measured when the fixture was written.)
FP32_ROUNDING = 2e-5


@pytest.fixture(scope="module")
def gold():
    return TO.load_golden()


@pytest.mark.parametrize("name", list(TO.CONFIGS))
def test_restatement_reproduces_the_hf_fixture(gold, name):
    cfg = TO.CONFIGS[name]
    assert int(gold[f"{name}.seed"]) == TO.SEEDS[name]
    sd = TO.make_weights(cfg, TO.SEEDS[name])
    ids, mask, mask_last = TO.make_ids_and_masks(cfg, TO.SEEDS[name])
    assert torch.equal(ids, torch.from_numpy(gold[f"{name}.ids"]))
    assert torch.equal(mask, torch.from_numpy(gold[f"{name}.mask"])) and torch.equal(mask_last, torch.from_numpy(gold[f"{name}.mask_last"]))
    assert mask.sum(dim=1).tolist() == [16, 5, 1] and int(mask_last[:, -1].sum()) == 0
    outs = {}
    for case in ("nomask", "mask", "mask_last"):
        m, last, pooled = TO.golden_case(gold, name, case)
        got = TO.forward(sd, cfg, ids, m)
        outs[case] = got
        assert float((got[0] - last.double()).abs().max()) <= FP32_ROUNDING, case
        assert float((got[1] - pooled.double()).abs().max()) <= FP32_ROUNDING, case
    # the mask matters (else the fixture would prove nothing about it), and a full-length row is untouched by it
    assert float((outs["mask"][1][1:] - outs["nomask"][1][1:]).abs().max()) > 1e-2
    assert float((outs["mask_last"][1] - outs["nomask"][1]).abs().max()) > 1e-3
    assert torch.equal(outs["mask"][0][0], outs["nomask"][0][0])


@pytest.mark.parametrize("name", list(TO.CONFIGS))
def test_restatement_matches_a_fresh_hf_model(name):
    pytest.importorskip("transformers")
    from tools.make_golden_text_tower import hf_model
    cfg = TO.CONFIGS[name]
    sd = TO.make_weights(cfg, 77)
    ids, mask, _ = TO.make_ids_and_masks(cfg, 77)
    m = hf_model(cfg, sd)
    with torch.no_grad():
        r = m(input_ids=ids, attention_mask=mask)
    want = TO.forward(sd, cfg, ids, mask)
    assert float((r.last_hidden_state.double() - want[0]).abs().max()) <= FP32_ROUNDING
    assert float((r.pooler_output.double() - want[1]).abs().max()) <= FP32_ROUNDING
    # the module under test carries HF's parameter names (a 4.x model holds them under "text_model.")
    import streamformer_amd as sa
    ours = sa.SiglipTextModel(sa.SiglipTextConfig(**cfg))
    theirs = {k[len("text_model."):] if k.startswith("text_model.") else k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == theirs


def test_package_exports_the_text_tower():
    import streamformer_amd
    assert issubclass(streamformer_amd.SiglipTextModel, torch.nn.Module)
    assert callable(streamformer_amd.encode_label_prompts) and callable(streamformer_amd.encode_captions)


def test_parameter_tree_packing_and_checkpoint_round_trip(tmp_path):
    import streamformer_amd as sa
    from streamformer_amd.text import normalize_text_keys, pack_qkv
    cfg = TO.CONFIGS["d128"]
    sd = TO.make_weights(cfg, 5)
    m = sa.SiglipTextModel(sa.SiglipTextConfig(**cfg))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == TO.weight_shapes(cfg)
    assert all(not p.requires_grad for p in m.parameters()) and not m.training
    assert m.device == torch.device("cpu")
    # keys with the 4.x prefix, next to a vision tower's and the model's scalars
    full = {"text_model." + k: v for k, v in sd.items()}
    full.update({"vision_model.post_layernorm.weight": torch.ones(3), "logit_scale": torch.zeros(1), "text_model.embeddings.position_ids": torch.arange(16)[None]})
    assert set(normalize_text_keys(full)) == set(sd)
    m.load_state_dict(full)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    w, b = pack_qkv(m.state_dict(), 1)
    D = cfg["hidden_size"]
    assert w.shape == (3 * D, D) and b.shape == (3 * D,)
    for i, n in enumerate("qkv"):
        assert torch.equal(w[i * D:(i + 1) * D], sd[f"encoder.layers.1.self_attn.{n}_proj.weight"])
        assert torch.equal(b[i * D:(i + 1) * D], sd[f"encoder.layers.1.self_attn.{n}_proj.bias"])
    # save / load, safetensors and .bin, flat config and a SiglipModel-style config with the fields under text_config
    for safe in (True, False):
        d = tmp_path / ("st" if safe else "bin")
        m.save_pretrained(str(d), safe_serialization=safe)
        back = sa.SiglipTextModel.from_pretrained(str(d), device="cpu")
        assert back.config.to_dict() == m.config.to_dict()
        for k, v in back.state_dict().items():
            assert torch.equal(v, sd[k]), k
    nested = tmp_path / "nested"
    m.save_pretrained(str(nested))
    flat = json.load(open(nested / "config.json"))
    json.dump({"model_type": "siglip", "text_config": flat, "vision_config": {"hidden_size": 8}}, open(nested / "config.json", "w"))
    assert sa.SiglipTextModel.from_pretrained(str(nested), device="cpu").config.to_dict() == m.config.to_dict()
    with pytest.raises(OSError, match="not a local directory"):
        sa.SiglipTextModel.from_pretrained(str(tmp_path / "absent"))


def test_python_refusals_carry_messages_and_launch_nothing():
    import streamformer_amd as sa
    cfg = TO.CONFIGS["d128"]
    m = sa.SiglipTextModel(sa.SiglipTextConfig(**cfg))          # on the CPU: a launch would need a device and fail differently
    ids = torch.zeros(2, 16, dtype=torch.long)
    with pytest.raises(ValueError, match=r"outside the vocabulary \[0, 97\)"):
        m(torch.full((2, 16), 97))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m(torch.tensor([[0, -1]]))
    with pytest.raises(ValueError, match="sequence length 17 exceeds max_position_embeddings 16"):
        m(torch.zeros(1, 17, dtype=torch.long))
    mask = torch.ones(2, 16, dtype=torch.long)
    mask[1] = 0
    with pytest.raises(ValueError, match="attention_mask row 1 has no valid key"):
        m(ids, attention_mask=mask)
    with pytest.raises(ValueError, match=r"attention_mask must be \[2, 16\]"):
        m(ids, attention_mask=torch.ones(2, 15))
    with pytest.raises(NotImplementedError, match="position_ids other than arange"):
        m(ids, position_ids=torch.arange(16).flip(0)[None].expand(2, 16))
    with pytest.raises(ValueError, match="specify input_ids"):
        m()
    with pytest.raises(ValueError, match="whole groups of 3"):
        m.encode_groups(ids, 3)
    assert m._handle is None                                      # nothing was packed, let alone launched
    with pytest.raises(ValueError, match="compute_dtype"):
        sa.SiglipTextModel(sa.SiglipTextConfig(**cfg), compute_dtype="fp16")
    with pytest.raises(ValueError, match="hidden_act"):
        sa.SiglipTextModel(sa.SiglipTextConfig(**dict(cfg, hidden_act="swish")))
    with pytest.raises(sa._native.NativeError, match="head_dim 12"):
        sa.SiglipTextModel(sa.SiglipTextConfig(**dict(cfg, hidden_size=192, num_attention_heads=16)))


def test_native_refusals_carry_messages_and_launch_nothing():
    import streamformer_amd._native as nat

    def create(**kw):
        base = dict(vocab=97, positions=16, hidden=128, layers=1, heads=2, intermediate=256, projection=128, act=1, eps=1e-6)
        base.update(kw)
        h = C.c_void_p()
        rc = nat.lib.sf_text_create(C.byref(nat.SfTextConfig(*base.values())), 0, C.byref(h))
        return rc, h, (nat.lib.sf_last_error() or b"").decode()

    for kw, code, word in ((dict(hidden=144, heads=2), nat.SF_ERR_INVALID, "multiple of 64"),
                           (dict(hidden=320, heads=2), nat.SF_ERR_INVALID, "head_dim 160"),
                           (dict(hidden=128, heads=3), nat.SF_ERR_INVALID, "not divisible"),
                           (dict(positions=129), nat.SF_ERR_CAPACITY, "129 positions > 128"),
                           (dict(hidden=8192, heads=64), nat.SF_ERR_CAPACITY, "hidden 8192"),
                           (dict(act=3), nat.SF_ERR_INVALID, "act code 3"),
                           (dict(vocab=0), nat.SF_ERR_INVALID, "positive")):
        rc, _, msg = create(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    for ok in (dict(), dict(hidden=576, heads=8, intermediate=1072, projection=576), dict(hidden=1152, heads=16, intermediate=4304, positions=64)):
        rc, h, msg = create(**ok)
        assert rc == 0, msg
        nat.lib.sf_text_destroy(h)
    rc, h, _ = create()
    assert nat.lib.sf_text_missing_weights(h) == 2 + 16 + 4 and b"head.weight" in nat.lib.sf_last_error()
    x = torch.zeros(4, 128)
    shape = (C.c_int64 * 2)(4, 128)
    assert nat.lib.sf_text_load_tensor(h, b"text_model.pooler.weight", x.data_ptr(), nat.SF_F32, shape, 2) == nat.SF_ERR_UNKNOWN_KEY
    assert nat.lib.sf_text_load_tensor(h, b"text_model.head.weight", x.data_ptr(), nat.SF_F32, shape, 2) == nat.SF_ERR_INVALID
    assert b"shape mismatch" in nat.lib.sf_last_error()
    assert nat.lib.sf_text_finalize(h, nat.SF_COMPUTE_BF16) == nat.SF_ERR_STATE and b"missing" in nat.lib.sf_last_error()
    n = C.c_size_t()
    assert nat.lib.sf_text_workspace_bytes(h, 2, 16, C.byref(n)) == nat.SF_ERR_STATE and b"sf_text_finalize" in nat.lib.sf_last_error()
    assert nat.lib.sf_text_forward(h, 0, 0, 2, 16, 0, 0, 0, 0, 0) == nat.SF_ERR_STATE
    nat.lib.sf_text_destroy(h)
    # the single operators check their shapes before they launch
    assert nat.lib.sf_op_text_attention(16, 0, 16, 1, 129, 2, 64, 0) == nat.SF_ERR_CAPACITY and b"outside 1..128" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_text_attention(16, 0, 16, 1, 0, 2, 64, 0) == nat.SF_ERR_CAPACITY
    assert nat.lib.sf_op_text_attention(16, 0, 16, 1, 16, 2, 12, 0) == nat.SF_ERR_INVALID and b"head_dim" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_text_attention(0, 0, 16, 1, 16, 2, 64, 0) == nat.SF_ERR_INVALID
    assert nat.lib.sf_op_text_pool(16, 4, 16, 128, 0, 0, 1e-6, 16, 0, 128, 3, 16, 16, 0) == nat.SF_ERR_INVALID and b"group 3" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_text_pool(16, 4, 16, 126, 0, 0, 1e-6, 16, 0, 128, 0, 16, 0, 0) == nat.SF_ERR_INVALID
    assert nat.lib.sf_op_text_pool(16, 4, 16, 8192, 0, 0, 1e-6, 16, 0, 128, 0, 16, 0, 0) == nat.SF_ERR_CAPACITY


def _stub_tokenizer(texts, **kw):
    ids = torch.zeros(len(texts), 64, dtype=torch.long)
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids)}


def test_wrapper_without_a_text_tower_is_what_it_was():
    import streamformer_amd as sa
    from tests.helpers import small_cfg
    cfg = small_cfg()
    tasks = {"TaskRetrieval": {}, "TaskLocalization": {"label2id": {"toy": {"run": 0, "jump": 1}}, "prompt_templates": ["a clip of {}."]},
             "TaskGrounding": {}}
    torch.manual_seed(0)
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, tasks)
    w.prepare_for_multi_tasks()
    assert not hasattr(w, "text_encoder") and w.text_tokenizer is None
    assert not any("text_encoder" in k for k in w.state_dict()) and not any("text_encoder" in n for n, _ in w.named_modules())
    for head in w.task_heads.values():
        assert head._text_encoder is None and head._text_tokenizer is None
    loc = w.task_heads["TaskLocalization"]
    assert loc.dataset_label_embeddings == {}                    # no tower: templates alone build nothing
    feats = torch.randn(2, cfg.hidden_size)
    assert w.task_heads["TaskRetrieval"]._caption_features({"text_features": feats}, "cpu") is feats
    with pytest.raises(RuntimeError, match="text_encoder and text_tokenizer"):
        w.task_heads["TaskGrounding"]._caption_features({"caption": ["a", "b"]}, "cpu")
    with pytest.raises(KeyError, match="text_features"):
        w.task_heads["TaskRetrieval"]._caption_features({}, "cpu")
    with pytest.raises(ValueError, match="go together"):
        sa.StreamformerForMultiTaskingSigLIP(cfg, tasks, text_tokenizer=_stub_tokenizer)


def test_wrapper_registers_the_tower_once_and_hands_it_to_every_head():
    import streamformer_amd as sa
    from tests.helpers import small_cfg
    cfg = small_cfg()
    tower = sa.SiglipTextModel(sa.SiglipTextConfig(**TO.CONFIGS["d128"]))
    tasks = {"TaskRetrieval": {}, "TaskLocalization": {"label2id": {"toy": {"run": 0}}}}
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, tasks, text_encoder=tower, text_tokenizer=_stub_tokenizer)
    w.prepare_for_multi_tasks()
    names = [n for n, _ in w.named_parameters() if "token_embedding" in n]
    assert names == ["text_encoder.embeddings.token_embedding.weight"]
    assert all(not p.requires_grad for p in w.text_encoder.parameters())
    for head in w.task_heads.values():
        assert head._text_encoder is tower and head._text_tokenizer is _stub_tokenizer
        assert not any("text" in k for k in head.state_dict())
    assert w.task_heads["TaskLocalization"].dataset_label_embeddings == {}      # no prompt_templates: tables still come from set_label_embeddings
