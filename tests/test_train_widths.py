"""The training step at head widths other than 64 (SigLIP-so400m: 1152 / 16 heads of 72, I = 4304, 14 x 14 patches): the generic-width
attention backward (sf_attention_generic_bwd.hip) against torch autograd, whole-model gradients of the trainer and of the public layers
against oracle/train_oracle.py, the optimizer path, and what the trainer still refuses.  Tolerances are those of tests/train_support.py."""
import math

import pytest
import torch

from streamformer_amd.configuration import StreamformerConfig
from tests.helpers import cosine, rel_l2, small_cfg
from tests.train_support import GRAD_COS, GRAD_REL_L2, OP_TOL, attn_ref, compare_grads, device, to_dev, trainer_and_oracle

pytestmark = pytest.mark.gpu

HD72W = dict(image_size=42, patch_size=14, num_frames=8, hidden_size=576, num_hidden_layers=2, num_attention_heads=8, intermediate_size=1072)
HD32 = dict(image_size=48, patch_size=16, num_frames=8, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256)
SO400M_LAYER = dict(image_size=196, patch_size=14, num_frames=4, hidden_size=1152, num_hidden_layers=1, num_attention_heads=16,
                    intermediate_size=4304)


# ---------------------------------------------------------------------------------------------------
# the attention backward alone
# ---------------------------------------------------------------------------------------------------
def _op(layout, qkv, o, d_o, nseq, L, seq_rows, heads, hd, causal, fn="sf_op_attention_bwd_hd"):
    import streamformer_amd._native as nat
    dev = device()
    D = heads * hd
    dq = torch.full(tuple(qkv.shape[:-1]) + (3 * D,), float("nan")).bfloat16().to(dev)
    qd, od, dod = qkv.to(dev), o.to(dev), d_o.to(dev)
    args = [qd.data_ptr(), od.data_ptr(), dod.data_ptr(), dq.data_ptr(), layout, nseq, L, seq_rows, heads]
    args += [hd, causal] if fn == "sf_op_attention_bwd_hd" else [causal]
    nat.check(getattr(nat.lib, fn)(*args, nat.current_stream_handle(dev)))
    torch.cuda.synchronize()
    return dq


def _check(dq, want, D):
    scale = float(want.abs().max())
    assert not torch.isnan(dq.float()).any()
    for i, name in enumerate("qkv"):
        e = float((dq[..., i * D:(i + 1) * D].double().cpu() - want[..., i * D:(i + 1) * D]).abs().max()) / scale
        assert e < OP_TOL, (name, e)


@pytest.mark.parametrize("hd", [8, 32, 72, 96, 128])
@pytest.mark.parametrize("L", [1, 9, 50, 196, 224])
def test_generic_spatial_attention_bwd_matches_autograd(hd, L):
    heads, nseq = 2, 2
    D = heads * hd
    g = torch.Generator().manual_seed(hd * 1000 + L)
    qkv = (torch.randn(nseq, L, 3 * D, generator=g) * 1.5).bfloat16()
    d_o = torch.randn(nseq, L, D, generator=g).bfloat16()
    o_ref, want = attn_ref(qkv.float(), d_o.float(), nseq, L, heads, hd, False)
    dq = _op(0, qkv, o_ref.bfloat16(), d_o, nseq, L, 1, heads, hd, 0)
    _check(dq, want, D)


@pytest.mark.parametrize("hd", [8, 32, 72, 96, 128])
@pytest.mark.parametrize("L", [1, 4, 16, 32])
@pytest.mark.parametrize("causal", [1, 0])
def test_generic_temporal_attention_bwd_matches_autograd(hd, L, causal):
    B, N, heads = 2, 3, 2
    D = heads * hd
    g = torch.Generator().manual_seed(hd * 100 + L + causal)
    qkv = (torch.randn(B, L, N, 3 * D, generator=g) * 1.5).bfloat16()      # token row of (b, t, n) = (b*L + t)*N + n
    d_o = torch.randn(B, L, N, D, generator=g).bfloat16()
    seq = qkv.float().permute(0, 2, 1, 3).reshape(B * N, L, 3 * D)
    o_ref, dref = attn_ref(seq, d_o.float().permute(0, 2, 1, 3).reshape(B * N, L, D), B * N, L, heads, hd, bool(causal))
    o = o_ref.reshape(B, N, L, D).permute(0, 2, 1, 3).contiguous().bfloat16()
    want = dref.reshape(B, N, L, 3 * D).permute(0, 2, 1, 3)
    dq = _op(1, qkv, o, d_o, B * N, L, N, heads, hd, causal)
    _check(dq, want, D)


@pytest.mark.parametrize("layout,L,causal", [(0, 196, 0), (0, 50, 0), (1, 16, 1), (1, 32, 0)])
def test_head_dim_64_entry_is_the_tuned_kernel(layout, L, causal):
    """sf_op_attention_bwd_hd at head_dim 64 runs the kernels of sf_op_attention_bwd: bit-identical results."""
    heads, hd = 2, 64
    D = heads * hd
    g = torch.Generator().manual_seed(L)
    shape = (2, L, D) if layout == 0 else (2, L, 3, D)
    qkv = (torch.randn(*shape[:-1], 3 * D, generator=g) * 1.5).bfloat16()
    o = torch.randn(*shape, generator=g).bfloat16()
    d_o = torch.randn(*shape, generator=g).bfloat16()
    nseq, rows = (2, 1) if layout == 0 else (6, 3)
    a = _op(layout, qkv, o, d_o, nseq, L, rows, heads, hd, causal)
    b = _op(layout, qkv, o, d_o, nseq, L, rows, heads, hd, causal, fn="sf_op_attention_bwd")
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------------
# whole model vs the oracle's autograd
# ---------------------------------------------------------------------------------------------------
def _cfg(kw, lora=True):
    return StreamformerConfig(enable_causal_temporal=True, add_lora_spatial=lora, **kw)


def _one_step(tr, orc, cfg, task_idx, B=2):
    from oracle import train_oracle as TO
    task, x, ti, _ = TO.schedule(cfg, B=B)[task_idx]
    want_loss = orc.loss(task, x, ti)
    want_loss.backward()
    dev = tr.device
    _, pooler = tr.forward(x.to(dev))
    loss, gp, gs = tr.loss_and_grad(task, pooler, to_dev(ti, dev))
    tr.grad(f"task_heads.{task}.logit_scale").add_(gs[0])
    tr.grad(f"task_heads.{task}.logit_bias").add_(gs[1])
    tr.backward(gp)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(want_loss)) < 2e-2 * abs(float(want_loss)), (float(loss), float(want_loss))


@pytest.mark.parametrize("task_idx", [0, 1])
@pytest.mark.parametrize("freeze", [True, False])
def test_hd72w_gradients_match_oracle(task_idx, freeze):
    """576 / 8 heads of 72, I = 1072 and 14 x 14 patches (588-long patch vectors): generic attention and pooling head, padded MLP and
    patch widths; LoRA with the spatial base frozen and trained."""
    cfg = _cfg(HD72W)
    tr, orc = trainer_and_oracle(cfg, freeze, seed=15, lora=True)
    _one_step(tr, orc, cfg, task_idx)
    compare_grads(tr, orc)


@pytest.mark.parametrize("task_idx", [0, 1])
def test_hd32_gradients_match_oracle(task_idx):
    cfg = _cfg(HD32)
    tr, orc = trainer_and_oracle(cfg, True, seed=13, lora=True)
    _one_step(tr, orc, cfg, task_idx)
    compare_grads(tr, orc)


@pytest.mark.parametrize("task_idx", [0, 1])
def test_so400m_layer_gradients_match_oracle(task_idx):
    """One so400m-width layer: 1152 / 16 heads of 72, I = 4304, 196 patches of 14 x 14, 4 frames, B = 2."""
    cfg = _cfg(SO400M_LAYER)
    tr, orc = trainer_and_oracle(cfg, True, seed=16, lora=True)
    _one_step(tr, orc, cfg, task_idx)
    compare_grads(tr, orc)


def test_hd72w_gradients_are_deterministic_and_state_dict_keeps_reference_shapes():
    from oracle import train_oracle as TO
    cfg = _cfg(HD72W)
    tr, _ = trainer_and_oracle(cfg, True, seed=15, lora=True)
    task, x, ti, _ = TO.schedule(cfg)[1]
    dev = tr.device

    def run():
        _, pooler = tr.forward(x.to(dev))
        _, gp, _ = tr.loss_and_grad(task, pooler, to_dev(ti, dev))
        tr.backward(gp)
        torch.cuda.synchronize()
    run()
    g1 = tr.grads.clone()
    tr.zero_grad()
    run()
    assert torch.equal(g1, tr.grads)
    sd = tr.state_dict()
    assert tuple(sd["encoder.layer.0.intermediate.dense.weight"].shape) == (1072, 576)
    assert tuple(sd["encoder.layer.1.output.dense.weight"].shape) == (576, 1072)
    assert tuple(sd["head.mlp.fc1.weight"].shape) == (1072, 576)
    assert tuple(sd["embeddings.patch_embeddings.projection.weight"].shape) == (576, 3, 14, 14)
    assert tuple(tr.grad("encoder.layer.0.intermediate.dense.bias").shape) == (1072,)


def test_hd72w_three_adamw_steps_track_the_oracle():
    """3 optimizer steps (alternating tasks, clipped gradients) on the trainer and on the oracle (torch autograd + torch.optim.AdamW): losses
    within 3 %, and the parameter displacement agreeing in direction and size on the elements whose first gradient is significant (Adam
    turns bf16 noise on near-zero gradients into full-size steps of random sign)."""
    from oracle import train_oracle as TO
    cfg = _cfg(HD72W)
    tr, orc = trainer_and_oracle(cfg, True, seed=15, lora=True, lr=1e-3, wd=0.05)
    dev = tr.device
    sched = TO.schedule(cfg, B=2)
    start = {k: v.detach().clone() for k, v in orc.named.items()}
    got, want, g0 = [], [], None
    for it in range(3):
        task, x, ti, _ = sched[it % len(sched)]
        want_loss = orc.loss(task, x, ti)
        want_loss.backward()
        if g0 is None:
            g0 = {k: v.detach().clone() for k, v in orc.grads().items()}
        torch.nn.utils.clip_grad_norm_(list(orc.named.values()), 1.0)
        orc.opt.step()
        orc.opt.zero_grad(set_to_none=True)
        want.append(float(want_loss.detach()))
        got.append(float(tr.micro_step(task, x.to(dev), to_dev(ti, dev), lr=1e-3, weight_decay=0.05, clip_grad=1.0)))
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    assert max(rel) < 3e-2, list(zip(got, want))
    sd = tr.state_dict()
    num = den = dot = 0.0
    for k, p0 in start.items():
        if p0.numel() < 64 or k not in g0:
            continue
        sig = (g0[k].abs() > 0.05 * g0[k].abs().max()).flatten()
        dw_o = (orc.named[k].detach() - p0).double().flatten()[sig]
        dw_h = (sd[k].cpu() - p0).double().flatten()[sig]
        dot += float(dw_o @ dw_h); num += float(dw_h @ dw_h); den += float(dw_o @ dw_o)
    cos = dot / (num ** 0.5 * den ** 0.5)
    assert cos > 0.97 and 0.9 < (num / den) ** 0.5 < 1.1, (cos, (num / den) ** 0.5)


# ---------------------------------------------------------------------------------------------------
# public layers
# ---------------------------------------------------------------------------------------------------
def test_autograd_module_at_hd72w_matches_oracle():
    """model.train(); loss(out).backward() at head_dim 72 -> .grad of every trainable parameter vs the oracle's autograd."""
    import streamformer_amd as sa
    from oracle import streamformer_oracle as O
    device()
    cfg = _cfg(HD72W, lora=False)
    sd = sa.make_state_dict(cfg, seed=15)
    m = sa.TimesformerMultiTaskingModelSigLIP(cfg)
    m.load_state_dict(sd)
    m.cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 3, 42, 42, generator=g)
    wp = torch.randn(2, 4, cfg.hidden_size, generator=g)
    wl = torch.randn(2, 4, 9, cfg.hidden_size, generator=g) * 0.1

    def loss_of(out, wp, wl):
        return (out["pooler_output"] * wp).sum() + (out["last_hidden_state"] * wl).sum()
    out = m(x.cuda())
    loss = loss_of(out, wp.cuda(), wl.cuda())
    loss.backward()
    torch.cuda.synchronize()
    osd = {k: v.clone().requires_grad_(m._named[k].requires_grad) for k, v in sd.items() if not k.endswith(".mask")}
    want = loss_of(O.forward_graph(osd, cfg, x), wp, wl)
    want.backward()
    assert abs(float(loss) - float(want)) < 2e-2 * abs(float(want)) + 1e-2
    for k, p in m._named.items():
        if not p.requires_grad:
            continue
        assert p.grad is not None, k
        wg = osd[k].grad
        if wg.numel() == 1 or float(wg.abs().max()) < 1e-6:
            continue
        assert rel_l2(p.grad, wg) < GRAD_REL_L2 and cosine(p.grad, wg) > GRAD_COS, (k, rel_l2(p.grad, wg), cosine(p.grad, wg))


def test_multitask_wrapper_at_hd72w_gives_the_trainer_gradients():
    """StreamformerForMultiTaskingSigLIP (LoRA, frozen spatial base) at head_dim 72: one retrieval loss.backward() fills the encoder's
    .grad with what StreamformerTrainer computes for the same batch."""
    import streamformer_amd as sa
    from oracle import train_oracle as TO
    dev = device()
    cfg = _cfg(HD72W)
    sd = sa.make_state_dict(cfg, seed=15, lora=True)
    model = sa.StreamformerForMultiTaskingSigLIP(cfg, {"TaskRetrieval": {}, "TaskLocalization": {"label2id": {"synthetic": {}}}})
    model.timesformer.load_state_dict(sd)
    model.prepare_for_multi_tasks()
    model.frozen_spatial()
    model.cuda().train()
    task, x, ti, _ = TO.schedule(cfg)[0]
    assert ti["kind"] == "retrieval"
    ls, _ = model(x.to(dev), multi_task_input={"task_name": "TaskRetrieval", "task_input": {"text_features": ti["text"].to(dev)}})
    ls["TaskRetrieval"].backward()
    torch.cuda.synchronize()
    tr, _ = trainer_and_oracle(cfg, True, seed=15, lora=True)
    _, pooler = tr.forward(x.to(dev))
    loss, gp, _ = tr.loss_and_grad(task, pooler, to_dev(ti, dev))
    tr.backward(gp)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ls["TaskRetrieval"])) < 1e-3 * abs(float(loss)) + 1e-5
    named = dict(model.timesformer.named_parameters())
    checked = 0
    for n in tr.parameter_names(trainable_only=True):
        if n not in named:
            continue
        p = named[n]
        assert p.requires_grad and p.grad is not None, n
        want = tr.grad(n)
        if want.numel() == 1 or float(want.abs().max()) < 1e-6:
            continue
        assert rel_l2(p.grad, want) < GRAD_REL_L2 and cosine(p.grad, want) > GRAD_COS, (n, rel_l2(p.grad, want))
        checked += 1
    assert checked > 20


# ---------------------------------------------------------------------------------------------------
# what the trainer still refuses
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,needle", [
    (dict(hidden_size=192, num_attention_heads=16), "head_dim 12"),
    (dict(hidden_size=320, num_attention_heads=2), "head_dim 160"),
    (dict(hidden_size=144, num_attention_heads=2), "multiple of 64"),
    (dict(hidden_size=1280, num_attention_heads=20, intermediate_size=256), "at most 16 heads"),
    (dict(image_size=256), "<= 224"),
])
def test_trainer_refuses_widths_beyond_its_limits(kw, needle):
    import streamformer_amd._native as nat
    from streamformer_amd.init_weights import make_state_dict
    from streamformer_amd.training import StreamformerTrainer
    dev = device()
    cfg = small_cfg(add_lora_spatial=True, num_hidden_layers=1, **kw)
    with pytest.raises(nat.NativeError) as ei:
        StreamformerTrainer(cfg, make_state_dict(cfg, seed=1, lora=True), ["retrieval"], device=dev)
    assert needle in str(ei.value), str(ei.value)


def test_attention_dropout_at_generic_width_is_refused_at_construction():
    from streamformer_amd.init_weights import make_state_dict
    from streamformer_amd.training import StreamformerTrainer
    dev = device()
    cfg = _cfg(HD72W)
    cfg.attention_probs_dropout_prob = 0.1
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        StreamformerTrainer(cfg, make_state_dict(cfg, seed=1, lora=True), ["retrieval"], device=dev)
    assert math.isclose(cfg.hidden_size / cfg.num_attention_heads, 72.0)
