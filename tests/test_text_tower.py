"""The native SigLIP text tower on the MI355X: its two new operators against the fp64 restatement (tests/text_tower_oracle.py), the
whole model against the HF fixture (tests/golden/f18_text_tower.npz) and the restatement, and the multitask wrapper with a stub
tokenizer.

Tolerances follow tests/test_stage_precision.py: each bound is a multiple of the PRECISION FLOOR of what it bounds — the error, against
fp64, of the same operator sequence in torch at the operand precision of the mode (fp32 for the fp32 kernels; hi + lo bf16 planes with the
lo * lo product dropped for the Linears of the accurate mode, see _reference; bf16-rounded operands of the layers' Linears with fp32
accumulation for the bf16 mode).  The floor is computed here, on the CPU, from
the inputs; never from the code under test.  MARGIN = 4 covers a different summation order and the tanh / exp approximations.
"""
import ctypes as C
import math

import pytest
import torch

from tests import text_tower_oracle as TO
from tests.helpers import EPS32, MARGIN, fp32_floor, gpu_device, maxabs, randn, small_cfg

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# 1. sf_op_text_attention
# ------------------------------------------------------------------------------------------------
def _masks(B, L):
    """none; valid lengths {L, ceil(L / 2), 1}, right-padded; the last key masked (at L = 1 that would leave a caption without any
    valid key, which the Python layer refuses: the case does not exist there)."""
    out = {"none": None}
    m = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate((L, (L + 1) // 2, 1)):
        m[b, :n] = 1
    out["lengths"] = m
    if L > 1:
        m = torch.ones(B, L, dtype=torch.uint8)
        m[:, L - 1] = 0
        out["last"] = m
    return out


def _attention(nat, dev, qkv, mask, heads, hd):
    B, L, _ = qkv.shape
    q = qkv.to(dev).contiguous()
    m = None if mask is None else mask.to(dev).contiguous()
    ctx = torch.full((B, L, heads * hd), float("nan"), dtype=torch.float32, device=dev)
    nat.check(nat.lib.sf_op_text_attention(q.data_ptr(), nat.ptr(m), ctx.data_ptr(), B, L, heads, hd, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("hd", [8, 64, 72, 128])
@pytest.mark.parametrize("L", [1, 7, 16, 17, 64, 77, 128])
def test_text_attention_vs_fp64(L, hd):
    import streamformer_amd._native as nat
    dev = gpu_device()
    B, heads = 3, 2
    qkv = randn(1800 + 131 * L + hd, B, L, 3 * heads * hd) * 1.5          # as tests/test_train_widths.py draws attention inputs
    for name, mask in _masks(B, L).items():
        want = TO.attention(qkv.double(), mask, heads)
        floor = fp32_floor(TO.attention(qkv, mask, heads), want)
        got = _attention(nat, dev, qkv, mask, heads, hd)
        assert not torch.isnan(got).any(), f"{name}: output elements left unwritten"
        err = maxabs(got, want)
        print(f"[text attention L={L} hd={hd} mask={name}] max-abs {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}")
        # measured on an MI355X: see DESIGN.md "Text tower" (largest ratio over all cases next to MARGIN there)
        assert err <= MARGIN * floor, (name, err, floor)
        again = _attention(nat, dev, qkv, mask, heads, hd)
        assert torch.equal(got, again), f"{name}: two runs differ"
        if mask is not None:
            # a masked key has weight exactly 0: changing its k and v rows changes nothing
            other = qkv.clone().reshape(B, L, 3, heads * hd)
            dead = (mask == 0)
            other[:, :, 1:][dead] = randn(5, int(dead.sum()), 2, heads * hd) * 3.0
            assert torch.equal(_attention(nat, dev, other.reshape(B, L, -1), mask, heads, hd), got), f"{name}: a masked key leaked"


# ------------------------------------------------------------------------------------------------
# 2. sf_op_text_pool
# ------------------------------------------------------------------------------------------------
# B = 6: a partial workgroup of 8 captions (and, at B = 9, a second one); P = 72 / 200: partial 64-column blocks; L = 5: row 4 is pooled
@pytest.mark.parametrize("B,L,D,P", [(6, 5, 128, 72), (9, 3, 576, 200), (3, 1, 64, 8)])
@pytest.mark.parametrize("G", [0, 1, 3])
def test_text_pool_vs_fp64(B, L, D, P, G):
    import streamformer_amd._native as nat
    dev = gpu_device()
    x = randn(1850 + B, B, L, D) * 1.5
    gamma, beta = 1.0 + 0.1 * randn(1, D), 0.1 * randn(2, D)
    w, b = randn(3, P, D) / math.sqrt(D), 0.1 * randn(4, P)
    want = TO.pool(x.double(), gamma.double(), beta.double(), 1e-6, w.double(), b.double(), G)
    floor = fp32_floor(TO.pool(x, gamma, beta, 1e-6, w, b, G), want)
    rows = B // G if G else B
    out = torch.full((rows, P), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.empty(B, P, dtype=torch.float32, device=dev)
    t = [v.to(dev).contiguous() for v in (x, gamma, beta, w, b)]
    nat.check(nat.lib.sf_op_text_pool(t[0].data_ptr(), B, L, D, t[1].data_ptr(), t[2].data_ptr(), 1e-6, t[3].data_ptr(), t[4].data_ptr(), P, G,
                                      out.data_ptr(), scratch.data_ptr(), nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    got = out.cpu()
    assert not torch.isnan(got).any()
    err = maxabs(got, want)
    print(f"[text pool B={B} L={L} D={D} P={P} G={G}] max-abs {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}")
    assert err <= MARGIN * floor
    if G:
        assert maxabs(got.norm(dim=-1), torch.ones(rows)) <= 4 * EPS32 * 4
    if L > 1:
        # the pooled row is row L - 1 and no other: every other position may hold anything
        x2 = x.clone()
        x2[:, :L - 1] = 1e3
        t0 = x2.to(dev).contiguous()
        out2 = torch.empty_like(out)
        nat.check(nat.lib.sf_op_text_pool(t0.data_ptr(), B, L, D, t[1].data_ptr(), t[2].data_ptr(), 1e-6, t[3].data_ptr(), t[4].data_ptr(), P, G,
                                          out2.data_ptr(), scratch.data_ptr(), nat.current_stream_handle(dev)))
        torch.cuda.synchronize()
        assert torch.equal(out2.cpu(), got)


# ------------------------------------------------------------------------------------------------
# 3. whole model
# ------------------------------------------------------------------------------------------------
_GOLD = {}
_FLOORS = {}
_TOWERS = {}


def _gold():
    if not _GOLD:
        _GOLD.update(TO.load_golden())
    return _GOLD


def _reference(name, case):
    """fp64 restatement and the two precision floors of one (config, mask case): computed once, shared, never changed."""
    key = (name, case)
    if key not in _FLOORS:
        cfg, seed = TO.CONFIGS[name], TO.SEEDS[name]
        sd = TO.make_weights(cfg, seed)
        ids = torch.from_numpy(_gold()[f"{name}.ids"])
        mask, hf_last, hf_pooled = TO.golden_case(_gold(), name, case)
        want = TO.forward(sd, cfg, ids, mask)
        # The accurate mode's floor was first taken at plain fp32 operands and the first run on an MI355X missed 4 x that floor by a
        # factor of 5.6 (d128, no mask, last_hidden_state: 3.57e-5 against a floor of 1.60e-6).  The reason is the mode's own operand
        # precision: its Linears multiply hi + lo bf16 planes (16 mantissa bits, 2^-17 relative, against fp32's 2^-24) and drop the
        # lo * lo product.  The same operator sequence in torch at THAT operand precision (bf16_operands="x3") loses 3.54e-5 on the
        # same case — the kernels sit at 1.01 x it — so the accurate mode is bounded by 4 x this floor, and by 1e-3 besides.
        x3 = TO.forward(sd, cfg, ids, mask, dtype=torch.float32, bf16_operands="x3")
        b16 = TO.forward(sd, cfg, ids, mask, dtype=torch.float32, bf16_operands=True)
        _FLOORS[key] = dict(ids=ids, mask=mask, want=want, hf=(hf_last, hf_pooled),
                            floor={"fp32": tuple(fp32_floor(x3[i], want[i]) for i in range(2)),
                                   "bf16": tuple(fp32_floor(b16[i], want[i]) for i in range(2))})
    return _FLOORS[key]


def _tower(name, mode):
    key = (name, mode)
    if key not in _TOWERS:
        import streamformer_amd as sa
        m = sa.SiglipTextModel(sa.SiglipTextConfig(**TO.CONFIGS[name]), compute_dtype=mode)
        m.load_state_dict(TO.make_weights(TO.CONFIGS[name], TO.SEEDS[name]))
        _TOWERS[key] = m.to(gpu_device())
    return _TOWERS[key]


@pytest.mark.parametrize("case", ["nomask", "mask", "mask_last"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(TO.CONFIGS))
def test_whole_tower_vs_fixture_and_fp64(name, mode, case):
    dev = gpu_device()
    ref = _reference(name, case)
    m = _tower(name, mode)
    out = m(ref["ids"].to(dev), attention_mask=None if ref["mask"] is None else ref["mask"].to(dev))
    torch.cuda.synchronize()
    assert out[0].shape == ref["want"][0].shape and out[1].shape == ref["want"][1].shape
    assert out.last_hidden_state is out[0] and out.pooler_output is out[1]
    for i, what in enumerate(("last_hidden_state", "pooler_output")):
        got = out[i].cpu()
        err, floor = maxabs(got, ref["want"][i]), ref["floor"][mode][i]
        hf_err, hf_own = maxabs(got, ref["hf"][i]), maxabs(ref["hf"][i], ref["want"][i])
        print(f"[text tower {name} {mode} {case}] {what}: vs fp64 {err:.3e}  floor {floor:.3e}  ratio {err / floor:.2f}  vs HF fp32 {hf_err:.3e}")
        # measured on an MI355X: see DESIGN.md "Text tower"
        assert err <= MARGIN * floor, (what, err, floor)
        assert hf_err <= MARGIN * floor + hf_own, (what, hf_err)          # the fixture sits hf_own away from fp64 itself
        if mode == "fp32":
            assert err <= 1e-3                                            # the project's bound on unit-scale outputs in the accurate mode
    again = m(ref["ids"].to(dev), attention_mask=None if ref["mask"] is None else ref["mask"].to(dev))
    assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1])
    tup = m(ref["ids"].to(dev), return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2


# ------------------------------------------------------------------------------------------------
# 4. the multitask wrapper with a stub tokenizer
# ------------------------------------------------------------------------------------------------
def stub_tokenizer(texts, return_tensors="pt", padding="max_length", max_length=64, truncation=True):
    """Words hashed into the 97-entry vocabulary (id 1 = padding), padded to the tower's 16 positions."""
    assert return_tensors == "pt" and padding == "max_length" and max_length == 64
    L = 16
    ids = torch.ones(len(texts), L, dtype=torch.long)
    mask = torch.zeros(len(texts), L, dtype=torch.long)
    for i, t in enumerate(texts):
        words = t.lower().split()[:L]
        for j, w in enumerate(words):
            ids[i, j] = 2 + sum((k + 1) * ord(ch) for k, ch in enumerate(w)) % 95
        mask[i, :len(words)] = 1
    return {"input_ids": ids, "attention_mask": mask}


def _wrapper(tasks):
    import streamformer_amd as sa
    from streamformer_amd.init_weights import make_state_dict
    cfg = small_cfg(num_frames=8)
    tower = sa.SiglipTextModel(sa.SiglipTextConfig(**TO.CONFIGS["d128"]))
    tower.load_state_dict(TO.make_weights(TO.CONFIGS["d128"], TO.SEEDS["d128"]))
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, tasks, text_encoder=tower, text_tokenizer=stub_tokenizer)
    w.timesformer.load_state_dict(make_state_dict(cfg, seed=8))
    w.cuda()
    w.prepare_for_multi_tasks()
    return cfg, w


@pytest.mark.parametrize("task", ["TaskRetrieval", "TaskGrounding"])
def test_captions_through_the_wrapper_equal_their_text_features(task):
    dev = gpu_device()
    cfg, w = _wrapper({task: {}})
    w.train()
    captions = ["a person opens the door", "two dogs run"]
    x = randn(1890, 2, 8, 3, cfg.image_size, cfg.image_size).to(dev)
    extra = {"label": torch.tensor([[0, 1, 1, 0, 0, 1, 0, 1], [1, 1, 0, 0, 1, 0, 0, 0]], device=dev).float()} if task == "TaskGrounding" else {}
    tok = stub_tokenizer(captions)
    feats = w.text_encoder(tok["input_ids"].to(dev), attention_mask=tok["attention_mask"].to(dev))[1]
    assert feats.shape == (2, cfg.hidden_size) and not feats.requires_grad
    results = []
    for ti in ({"caption": captions}, {"text_features": feats}):
        w.zero_grad(set_to_none=True)
        losses, _ = w(x, multi_task_input={"task_name": task, "task_input": dict(ti, **extra)})
        losses[task].backward()
        torch.cuda.synchronize()
        results.append((losses[task].detach().clone(), {n: p.grad.clone() for n, p in w.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = results
    assert torch.equal(l0, l1) and torch.isfinite(l0)
    assert set(g0) == set(g1) and len(g0) > 10 and not any(n.startswith("text_encoder") for n in g0)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_localization_table_from_templates_equals_encode_label_prompts():
    import streamformer_amd as sa
    dev = gpu_device()
    templates = ["a clip of someone {}.", "footage showing {} outdoors"]
    labels = {"toy": {"running": 0, "high jump": 1, "opening a door": 2}, "given": {"x": 0}}
    cfg, w = _wrapper({"TaskRetrieval": {}})          # a wrapper only for its tower
    given = torch.nn.functional.normalize(randn(3, 1, cfg.hidden_size), dim=-1)
    import streamformer_amd.multitask as mt
    head = mt.TimesformerUniversalLocalizationHead(cfg, labels, prompt_templates=templates)
    head.set_label_embeddings("given", given)
    head.prepare_multi_task(w.text_encoder, stub_tokenizer, w.logit_scale, w.logit_bias, w.timesformer)
    assert torch.equal(head.dataset_label_embeddings["given"], given)          # a table that was set is kept
    table = head.dataset_label_embeddings["toy"]
    direct = sa.encode_label_prompts(w.text_encoder, stub_tokenizer, list(labels["toy"]), templates)
    assert table.shape == (3, cfg.hidden_size) and torch.equal(table, direct)
    # ... and both are the prompt-ensemble rule on the tower's own pooled rows: normalise, mean over the templates, normalise
    texts = [t.format(label) for label in labels["toy"] for t in templates]
    pooled = w.text_encoder(stub_tokenizer(texts)["input_ids"].to(dev))[1].double().cpu()
    want = TO.pool(pooled[:, None, :], None, None, 0.0, torch.eye(cfg.hidden_size, dtype=torch.float64), None, group=2)
    assert maxabs(table, want) <= MARGIN * 4 * EPS32          # unit-norm rows: a few fp32 roundings of entries below 1
    assert maxabs(table.norm(dim=-1), torch.ones(3)) <= 16 * EPS32
