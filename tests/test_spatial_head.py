"""The spatial task: video instance segmentation head (fused mask loss ``sf_mask_loss``, dense projection ``sf_dense_head_*``),
and the zero-shot classification head — against tests/spatial_head_oracle.py, which tools/make_golden_spatial_head.py pins to the
reference (fixture F16, tests/golden/f16_vis_head.npz: the reference's own tensors).

Gradient bound of the loss kernel.  The yardstick is the fp32 floor recorded in F16: the reference's operator sequence evaluated
in fp32 against the fp64 restatement on the same inputs, max-abs error over the tensor's max-abs.  Measured on the CPU by the
generator: d dense 7.8e-7 (case a), 7.8e-7 (b), 1.3e-6 (c), 2.3e-6 (benchmark-sized clip, 16 x 196 x 768, L = 100, 224 x 398);
d (logit_scale, logit_bias) 8.9e-8, 5.4e-8, 1.1e-7, 2.0e-7.  The kernel is allowed 8 x the floor of the same inputs: it adds a
patch's pixels in another order than torch and uses the hardware exponential.  A wrong interpolation weight shows at 1e-2.
Measured kernel errors: DESIGN.md §6, "Spatial task".
"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from tests import spatial_head_oracle as S
from tests.helpers import cosine, load_npz, maxabs, rel_l2, small_cfg

T_FRAMES = 4
FLOOR_FACTOR = 8.0
LOSS_TOL = 2e-5            # the F6 bound of test_hip_parity.py
# edge cases without a recorded floor of their own: the largest floor measured on small inputs (case c)
SMALL_FLOOR_KEY = "c_floor"


def f16_cfg():
    return small_cfg(intermediate_size=64, num_frames=T_FRAMES)


@pytest.fixture(scope="module")
def f16(golden_dir):
    return load_npz(os.path.join(golden_dir, "f16_vis_head.npz"))


# local: unlike helpers.rel_max it has no guard in the denominator, so an all-zero reference fails instead of passing
def relmax(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def head_weights(f16):
    """The ten projection tensors of the fixture: regenerated from the seed, checked against the recorded digest."""
    from streamformer_amd.init_weights import make_state_dict, state_dict_sha256
    cfg = f16_cfg()
    sd = make_state_dict(cfg, seed=int(f16["weights_seed"]))
    assert state_dict_sha256(sd) == str(f16["state_dict_sha256"]), "RNG drift: the seeded weights differ from the fixture's"
    D = cfg.hidden_size
    vals = (sd["head.attention.in_proj_weight"][2 * D:], sd["head.attention.in_proj_bias"][2 * D:], sd["head.attention.out_proj.weight"],
            sd["head.attention.out_proj.bias"], sd["head.layernorm.weight"], sd["head.layernorm.bias"], sd["head.mlp.fc1.weight"],
            sd["head.mlp.fc1.bias"], sd["head.mlp.fc2.weight"], sd["head.mlp.fc2.bias"])
    return {n: v.clone() for n, v in zip(S.PROJ_NAMES, vals)}, sd


def case_inputs(f16, tag):
    cfg = f16_cfg()
    datasets = [str(d) for d in f16[f"{tag}_datasets"]]
    lhs = S.seeded_randn(int(f16[f"{tag}_lhs_seed"]), len(datasets), T_FRAMES, cfg.num_patches, cfg.hidden_size)
    assert abs(float(lhs.double().sum()) - float(f16[f"{tag}_lhs_sum"])) < 1e-6, "RNG drift: seeded inputs differ from the fixture's"
    masks = [torch.from_numpy(f16[f"{tag}_mask{i}"].astype(np.int64)) for i in range(len(datasets))]
    sizes = [tuple(int(v) for v in s) for s in f16[f"{tag}_mask_sizes"]]
    tables = {d: torch.from_numpy(f16[f"table_{d}"]) for d in set(datasets)}
    seed = int(f16[f"{tag}_random_seed"]) if f"{tag}_random_seed" in f16 else None
    return cfg, datasets, lhs, masks, sizes, tables, seed


def selected(f16, tag):
    """Per-clip (table, remapped target) of the recorded draw, and the dense embeddings the loss kernel is fed (fp64 restatement)."""
    cfg, datasets, lhs, masks, sizes, tables, seed = case_inputs(f16, tag)
    if seed is not None:
        random.seed(seed)
    sel = [S.select_classes(tables[d], masks[i]) for i, d in enumerate(datasets)]
    for i, (_, t) in enumerate(sel):
        assert torch.equal(t, torch.from_numpy(f16[f"{tag}_sel_target{i}"].astype(np.int64))), "class draw differs from the recorded one"
    p, _ = head_weights(f16)
    dense = S.dense_projection(lhs.double(), {k: v.double() for k, v in p.items()}, cfg.layer_norm_eps).float()
    return dense, [t for t, _ in sel], [m for _, m in sel]


def fp64_mask_loss(x, tables, targets, ls=np.log(10.0), lb=-2.0, device="cpu"):
    xd = x.detach().to(device, torch.float64).requires_grad_(True)
    s = torch.tensor(ls, dtype=torch.float64, device=device, requires_grad=True)
    b = torch.tensor(lb, dtype=torch.float64, device=device, requires_grad=True)
    loss = S.mask_loss(xd, [t.to(device, torch.float64) for t in tables], [t.to(device) for t in targets], s, b)
    loss.backward()
    gx = xd.grad if xd.grad is not None else torch.zeros_like(xd)
    gs = torch.stack([s.grad if s.grad is not None else torch.zeros_like(s), b.grad if b.grad is not None else torch.zeros_like(b)])
    return loss.detach(), gx, gs


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_matches_reference_fixture(f16, tag):
    cfg, datasets, lhs, masks, sizes, tables, seed = case_inputs(f16, tag)
    p, _ = head_weights(f16)
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    lhs.requires_grad_(True)
    ls = torch.log(torch.tensor(10.0)).requires_grad_(True)
    lb = torch.tensor(-2.0).requires_grad_(True)
    if seed is not None:
        random.seed(seed)
    loss = S.vis_head_loss(lhs, p, cfg.layer_norm_eps, tables, datasets, masks, sizes, cfg.image_size, ls, lb)
    loss.backward()
    assert maxabs(loss.detach(), f16[f"{tag}_loss"]) < 1e-5
    assert maxabs(lhs.grad, f16[f"{tag}_d_lhs"]) < 1e-6
    assert maxabs(ls.grad, f16[f"{tag}_d_logit_scale"]) < 1e-6 and maxabs(lb.grad, f16[f"{tag}_d_logit_bias"]) < 1e-6
    for n in S.PROJ_NAMES:
        assert maxabs(p[n].grad, f16[f"{tag}_d_{n}"]) < 1e-6, n
    if tag == "b":       # the all-background clip: loss 0, no gradient, still counted in the mean
        assert float(lhs.grad[1].abs().max()) == 0.0 and float(lhs.grad[0].abs().max()) > 0


def test_classification_restatement_matches_reference_fixture(f16):
    p = torch.from_numpy(f16["d_pooler"]).requires_grad_(True)
    ls = torch.log(torch.tensor(10.0)).requires_grad_(True)
    lb = torch.tensor(-2.0).requires_grad_(True)
    loss = S.classification_loss(p, torch.from_numpy(f16["d_table"]), torch.from_numpy(f16["d_labels"]), ls, lb)
    loss.backward()
    assert maxabs(loss.detach(), f16["d_loss"]) < 1e-5 and maxabs(p.grad, f16["d_d_pooler"]) < 1e-6
    assert maxabs(ls.grad, f16["d_d_logit_scale"]) < 1e-6 and maxabs(lb.grad, f16["d_d_logit_bias"]) < 1e-6
    assert float(p.grad[:, :-1].abs().max()) == 0.0


def test_class_subsampling_replays_the_recorded_draw(f16):
    from streamformer_amd.multitask import select_vis_classes
    cfg, datasets, lhs, masks, sizes, tables, seed = case_inputs(f16, "c")
    random.seed(seed)
    for i, d in enumerate(datasets):             # module-level generator, clip after clip, as the reference draws
        rows, tgt = select_vis_classes(tables[d], masks[i])
        assert rows.shape[0] == 100 and torch.equal(tgt, torch.from_numpy(f16[f"c_sel_target{i}"].astype(np.int64)))
        assert torch.allclose(rows.norm(dim=-1), torch.ones(100), atol=1e-6)
    rng = random.Random(seed)                    # the same draw through an explicit generator
    rows2, tgt2 = select_vis_classes(tables[datasets[0]], masks[0], rng)
    assert torch.equal(tgt2, torch.from_numpy(f16["c_sel_target0"].astype(np.int64)))
    small, tgt = select_vis_classes(tables[datasets[0]][:12] * 2.0, masks[0].clamp(max=11))
    assert torch.equal(small, tables[datasets[0]][:12] * 2.0)          # at most 100 classes: used as given, not normalised
    assert int((tgt == 0).sum()) == 0 and int((tgt == -1).sum()) == int((masks[0] == 0).sum())


def test_mask_loss_workspace_never_holds_the_upsampled_logits():
    import streamformer_amd._native as nat
    T, N, L, H, W = 16, 196, 100, 224, 398
    ws = nat.lib.sf_mask_loss_workspace_bytes(1, T, N, L)
    assert 0 < ws < T * L * H * W * 4 / 10, ws
    # grows with B T N L only
    assert nat.lib.sf_mask_loss_workspace_bytes(2, T, N, L) <= 2 * ws


def test_mask_loss_refuses_unsupported_shapes_with_a_message():
    """Capacity / shape errors come back as codes before anything is launched (no GPU needed: the pointers are never used)."""
    import streamformer_amd._native as nat

    def call(B=1, T=2, N=9, D=64, L=5, W=48, H=48, ws=1 << 20):
        one = ctypes.c_void_p(256)
        tp, mp = (ctypes.c_void_p * B)(*[256] * B), (ctypes.c_void_p * B)(*[256] * B)
        nl, wd = (ctypes.c_int32 * B)(*[L] * B), (ctypes.c_int32 * B)(*[W] * B)
        return nat.lib.sf_mask_loss(one, B, T, N, D, tp, nl, mp, wd, H, one, one, one, None, None, one, ws, None)
    assert call(N=256) == nat.SF_ERR_CAPACITY and b"224" in nat.lib.sf_last_error()
    assert call(N=10) == nat.SF_ERR_INVALID and b"square" in nat.lib.sf_last_error()
    assert call(L=129) == nat.SF_ERR_CAPACITY and b"label classes" in nat.lib.sf_last_error()
    assert call(W=4 * 48 + 1) == nat.SF_ERR_CAPACITY and b"mask width" in nat.lib.sf_last_error()
    assert call(D=4096) == nat.SF_ERR_CAPACITY and b"feature width" in nat.lib.sf_last_error()
    assert call(ws=16) == nat.SF_ERR_WORKSPACE and b"workspace" in nat.lib.sf_last_error()
    assert call(L=0) == nat.SF_ERR_INVALID
    assert nat.lib.sf_dense_head_forward(None, 8, 100, 64, 1e-6, None, None, None, 0, None) == nat.SF_ERR_INVALID
    assert b"multiple of 64" in nat.lib.sf_last_error()


def test_wrapper_builds_the_vis_and_classification_heads(f16):
    """Fails on a tree without the feature (NotImplementedError for both task types)."""
    import streamformer_amd as sa
    from streamformer_amd.multitask import (TimesformerUniversalVideoInstanceSegmentationHead, TimesformerVideoClassificationHead)
    cfg = f16_cfg()
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, {"TaskVIS": {"label2id": {"vis12": {}}}, "Kinetics": {"label2id": {}}})
    vis, cls = w.task_heads["TaskVIS"], w.task_heads["Kinetics"]
    assert isinstance(vis, TimesformerUniversalVideoInstanceSegmentationHead) and isinstance(cls, TimesformerVideoClassificationHead)
    _, sd = head_weights(f16)
    w.timesformer.load_state_dict(sd)
    w.prepare_for_multi_tasks()
    assert [n for n, _ in vis.named_parameters()] == [str(n) for n in f16["vis_param_names"]]
    assert [p.requires_grad for _, p in vis.named_parameters()] == [bool(v) for v in f16["vis_param_requires_grad"]]
    p, _ = head_weights(f16)
    named = dict(vis.named_parameters())
    for n in S.PROJ_NAMES:                       # deep copies of the pooling head's tensors (modeling:1764-1779), not views
        assert torch.equal(named[n].detach(), p[n]), n
    assert named["w_v.weight"].data_ptr() != w.timesformer.head.attention.in_proj_weight.data_ptr()
    assert named["head.probe"] is w.timesformer.head.probe             # the registered pooling head is the encoder's own (shared)
    names = [n for n, _ in w.named_parameters()]
    assert len(names) == len(set(names)) and "task_heads.TaskVIS.w_v.weight" in names and "task_heads.TaskVIS.head.probe" not in names
    for other in ("YoutubeVIS", "LVVIS", "COCOPseudoVIS"):
        assert isinstance(sa.StreamformerForMultiTaskingSigLIP(cfg, {other: {"label2id": {}}}).task_heads[other],
                          TimesformerUniversalVideoInstanceSegmentationHead)
    vis.eval()
    assert vis(None, {}) is None                 # as the reference: no evaluation output


# ------------------------------------------------------------------------------------------------ GPU
# local: this file is not marked gpu as a whole, so a missing GPU skips here where helpers.gpu_device() asserts
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def run_mask_loss(x, tables, targets, need_grad=True):
    from streamformer_amd.heads import MaskLossHead
    dev = torch.device("cuda")
    loss, gx, gs = MaskLossHead().loss(x.to(dev), [t.to(dev) for t in tables], [t.to(dev) for t in targets], need_grad=need_grad)
    torch.cuda.synchronize()
    return loss, gx, gs


def check_mask_loss(x, tables, targets, floor, what):
    loss, gx, gs = run_mask_loss(x, tables, targets)
    want, wgx, wgs = fp64_mask_loss(x, tables, targets, device="cuda" if x.numel() > 1 << 20 else "cpu")
    e_loss, e_gx, e_gs = abs(float(loss) - float(want)), relmax(gx, wgx), relmax(gs, wgs)
    print(f"{what}: loss {float(loss):.6f} err {e_loss:.2e} | d dense {e_gx:.2e} (floor {floor[1]:.2e}) | d scalars {e_gs:.2e} (floor {floor[2]:.2e})"
          f" [d scale {float(gs[0]):.6e} want {float(wgs[0]):.6e}, d bias {float(gs[1]):.3e} want {float(wgs[1]):.3e}]")
    assert e_loss < LOSS_TOL, (what, e_loss)
    assert e_gx <= FLOOR_FACTOR * floor[1], (what, e_gx, floor[1])
    assert e_gs <= FLOOR_FACTOR * floor[2], (what, e_gs, floor[2])
    return loss, gx, gs


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_mask_loss_kernel_vs_fp64_on_the_fixture_inputs(f16, tag):
    _gpu()
    dense, tables, targets = selected(f16, tag)
    _, gx, _ = check_mask_loss(dense, tables, targets, f16[f"{tag}_floor"], f"F16 {tag}")
    if tag == "b":
        assert float(gx[1].abs().max()) == 0.0


@pytest.mark.gpu
def test_mask_loss_kernel_vs_fp64_on_a_benchmark_sized_clip(f16):
    _gpu()
    x, table, target = S.bench_clip_inputs()
    check_mask_loss(x[None], [table], [target], f16["bench_floor"], "16 x 196 x 768, L = 100, 224 x 398")


def _edge(seed, T, P, D, L, H, W, valid=None):
    x = S.seeded_randn(seed, 1, T, P * P, D)
    table = S.unit_rows(L, D, seed + 1)
    target = S.blocky_mask(seed + 2, T, H, W, list(range(L)), cells=5)
    if valid is not None:
        keep = torch.zeros_like(target, dtype=torch.bool)
        keep[valid] = True
        target = torch.where(keep, target, torch.full_like(target, -1))
    return x, [table], [target]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [
    ("W < H", dict(T=2, P=3, D=128, L=7, H=48, W=20)),
    ("W > H", dict(T=2, P=3, D=128, L=7, H=48, W=131)),
    ("last row only", dict(T=2, P=3, D=128, L=7, H=48, W=60, valid=(slice(None), slice(47, 48), slice(None)))),
    ("last column only", dict(T=2, P=3, D=128, L=7, H=48, W=60, valid=(slice(None), slice(None), slice(59, 60)))),
    ("L = 1", dict(T=2, P=3, D=128, L=1, H=48, W=48)),
    ("L = 128", dict(T=2, P=3, D=128, L=128, H=48, W=48)),
    ("N = 196", dict(T=2, P=14, D=192, L=9, H=224, W=300)),
])
def test_mask_loss_edge_cases(f16, name, kw):
    _gpu()
    x, tables, targets = _edge(1700, **kw)
    if kw["L"] == 1:       # one class: every logit gradient cancels (softmax = 1 = one-hot); compare absolutely
        loss, gx, gs = run_mask_loss(x, tables, targets)
        assert abs(float(loss)) < LOSS_TOL and float(gx.abs().max()) < 1e-6 and float(gs.abs().max()) < 1e-6
        return
    check_mask_loss(x, tables, targets, f16[SMALL_FLOOR_KEY], name)


@pytest.mark.gpu
def test_mask_loss_all_ignore_clip_inside_a_batch_and_null_gradients(f16):
    _gpu()
    x = S.seeded_randn(1710, 3, 2, 9, 128)
    tables = [S.unit_rows(6, 128, 1711), S.unit_rows(11, 128, 1712), S.unit_rows(6, 128, 1713)]
    targets = [S.blocky_mask(1714, 2, 48, 52, range(6)), torch.full((2, 48, 70), -1, dtype=torch.long), S.blocky_mask(1715, 2, 48, 31, range(6))]
    loss, gx, gs = check_mask_loss(x, tables, targets, f16[SMALL_FLOOR_KEY], "all-ignore clip in a batch of 3")
    assert float(gx[1].abs().max()) == 0.0 and float(gx[0].abs().max()) > 0 and float(gx[2].abs().max()) > 0
    loss2, gx2, gs2 = run_mask_loss(x, tables, targets, need_grad=False)            # NULL gradient pointers
    assert gx2 is None and gs2 is None and torch.equal(loss2, loss)


@pytest.mark.gpu
def test_mask_loss_is_bit_reproducible(f16):
    _gpu()
    dense, tables, targets = selected(f16, "a")
    a = run_mask_loss(dense, tables, targets)
    b = run_mask_loss(dense, tables, targets)
    x, table, target = S.bench_clip_inputs(T=4)
    c = run_mask_loss(x[None], [table], [target])
    d = run_mask_loss(x[None], [table], [target])
    for p, q in zip(a + c, b + d):
        assert torch.equal(p, q)


@pytest.mark.gpu
@pytest.mark.parametrize("I", [64, 200])
def test_dense_projection_forward_backward_vs_restatement(f16, I):
    _gpu()
    from streamformer_amd.heads import DenseHeadProjection
    cfg = f16_cfg()
    D = cfg.hidden_size
    if I == 64:
        p, _ = head_weights(f16)
    else:                  # an intermediate size that is not a multiple of 64 (zero-padded inside)
        from streamformer_amd.init_weights import make_state_dict
        sd = make_state_dict(small_cfg(intermediate_size=I, num_frames=T_FRAMES), seed=17)
        p = {n: v for n, v in zip(S.PROJ_NAMES, (sd["head.attention.in_proj_weight"][2 * D:], sd["head.attention.in_proj_bias"][2 * D:],
                                                 sd["head.attention.out_proj.weight"], sd["head.attention.out_proj.bias"], sd["head.layernorm.weight"],
                                                 sd["head.layernorm.bias"], sd["head.mlp.fc1.weight"], sd["head.mlp.fc1.bias"],
                                                 sd["head.mlp.fc2.weight"], sd["head.mlp.fc2.bias"]))}
    x = S.seeded_randn(1720, 2, T_FRAMES, 9, D)
    g = S.seeded_randn(1721, 2, T_FRAMES, 9, D)
    proj = DenseHeadProjection(cfg.layer_norm_eps)
    out = proj.forward(x.cuda(), [p[n].cuda() for n in S.PROJ_NAMES])
    dx, grads = proj.backward(g.cuda())
    torch.cuda.synchronize()
    pr = {n: v.clone().requires_grad_(True) for n, v in p.items()}
    xr = x.clone().requires_grad_(True)
    want = S.dense_projection(xr, pr, cfg.layer_norm_eps)
    (want * g).sum().backward()
    assert rel_l2(out, want.detach()) < 2e-2
    for name, got, ref in [("d x", dx, xr.grad)] + [(n, gg, pr[n].grad) for n, gg in zip(S.PROJ_NAMES, grads)]:
        r, c = rel_l2(got, ref), cosine(got, ref)
        print(f"dense projection I={I} {name}: rel L2 {r:.2e} cosine {c:.5f}")
        assert r <= 5e-2 and c >= 0.998, (name, r, c)


def _vis_model(f16, tasks):
    import streamformer_amd as sa
    cfg = f16_cfg()
    _, sd = head_weights(f16)
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, tasks)
    w.timesformer.load_state_dict(sd)
    w.prepare_for_multi_tasks()
    return cfg, sd, w.cuda().train()


@pytest.mark.gpu
def test_vis_batch_through_the_wrapper_vs_oracle_autograd(f16):
    _gpu()
    from oracle import streamformer_oracle as O
    cfg, sd, w = _vis_model(f16, {"TaskVIS": {"label2id": {"vis12": {}}}})
    _, datasets, _, masks, sizes, tables, _ = case_inputs(f16, "a")
    w.task_heads["TaskVIS"].set_label_embeddings("vis12", tables["vis12"])
    x = S.seeded_randn(1730, 2, T_FRAMES, 3, 48, 48)
    losses, _ = w(x.cuda(), multi_task_input={"task_name": "TaskVIS", "task_input": {"dataset": datasets, "mask_target": masks, "mask_size": sizes}})
    losses["TaskVIS"].backward()
    torch.cuda.synchronize()
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.endswith(".mask")}
    p, _ = head_weights(f16)
    pr = {n: v.clone().requires_grad_(True) for n, v in p.items()}
    ls = torch.log(torch.tensor(10.0)).requires_grad_(True)
    lb = torch.tensor(-2.0).requires_grad_(True)
    out = O.forward_graph(osd, cfg, x)
    want = S.vis_head_loss(out["last_hidden_state"], pr, cfg.layer_norm_eps, tables, datasets, masks, sizes, cfg.image_size, ls, lb)
    want.backward()
    assert abs(float(losses["TaskVIS"]) - float(want)) < 2e-2 * abs(float(want)) + 1e-2
    head = dict(w.task_heads["TaskVIS"].named_parameters())
    compared, pooled = 0, 0
    for k, pm in w.timesformer._named.items():
        assert pm.grad is not None, k
        if k.startswith("head."):                          # probe, pooling attention, its MLP: nothing of this task reaches them
            assert float(pm.grad.abs().max()) == 0.0, k
            pooled += 1
            continue
        wg = osd[k].grad
        assert wg is not None and float(wg.abs().max()) > 1e-6, (k, "every encoder parameter below the pooling head feeds last_hidden_state")
        if wg.numel() == 1:                                # temporal gates: one number, no direction to take a cosine of
            assert abs(float(pm.grad) - float(wg)) < 5e-2 * abs(float(wg)), (k, float(pm.grad), float(wg))
        else:
            r, c = rel_l2(pm.grad, wg), cosine(pm.grad, wg)
            assert r < 5e-2 and c > 0.998, (k, r, c)
        compared += 1
    assert pooled == 11 and compared == len(w.timesformer._named) - pooled, (compared, pooled)      # nothing dropped out of the loop
    for n in S.PROJ_NAMES:
        r, c = rel_l2(head[n].grad, pr[n].grad), cosine(head[n].grad, pr[n].grad)
        assert r < 5e-2 and c > 0.998, (n, r, c)
    assert abs(float(head["logit_scale"].grad) - float(ls.grad)) < 5e-2 * abs(float(ls.grad)), (float(head["logit_scale"].grad), float(ls.grad))
    # d logit_bias is mathematically zero (a shift of every logit of a pixel cancels in the softmax); the kernel's own figure is tested
    # against the fp32 floor in the sf_mask_loss tests above


@pytest.mark.gpu
def test_kinetics_batch_matches_the_reference_fixture(f16):
    dev = _gpu()
    from streamformer_amd.modeling import ModelOutput
    cfg, sd, w = _vis_model(f16, {"Kinetics": {"label2id": {}}})
    head = w.task_heads["Kinetics"]
    head.set_label_embeddings(torch.from_numpy(f16["d_table"]))
    pooler = torch.from_numpy(f16["d_pooler"]).to(dev).requires_grad_(True)
    loss, logits = head(ModelOutput(pooler_output=pooler), {"label": torch.from_numpy(f16["d_labels"])})
    loss.backward()
    torch.cuda.synchronize()
    # the F6 bounds of tests/test_hip_parity.py for the same kernel: loss 2e-5, d pooler 1e-6 max-abs, scalars 2e-5
    print(f"Kinetics vs F16 d: loss err {maxabs(loss.detach(), f16['d_loss']):.2e}, d pooler err {maxabs(pooler.grad, f16['d_d_pooler']):.2e}, "
          f"d scale err {maxabs(head.logit_scale.grad, f16['d_d_logit_scale']):.2e}, d bias err {maxabs(head.logit_bias.grad, f16['d_d_logit_bias']):.2e}")
    assert maxabs(loss.detach(), f16["d_loss"]) < 2e-5 and maxabs(pooler.grad, f16["d_d_pooler"]) < 1e-6
    assert maxabs(head.logit_scale.grad, f16["d_d_logit_scale"]) < 2e-5 and maxabs(head.logit_bias.grad, f16["d_d_logit_bias"]) < 2e-5
    assert float(pooler.grad[:, :-1].abs().max()) == 0.0 and logits.shape == (3, 10)


@pytest.mark.gpu
def test_adamw_steps_alternating_vis_and_retrieval(f16):
    _gpu()
    cfg, sd, w = _vis_model(f16, {"TaskVIS": {"label2id": {"vis12": {}}}, "TaskRetrieval": {}})
    _, datasets, _, masks, sizes, tables, _ = case_inputs(f16, "a")
    w.task_heads["TaskVIS"].set_label_embeddings("vis12", tables["vis12"])
    x = S.seeded_randn(1740, 2, T_FRAMES, 3, 48, 48).cuda()
    text = S.seeded_randn(1741, 2, cfg.hidden_size).cuda()
    vis_in = {"task_name": "TaskVIS", "task_input": {"dataset": datasets, "mask_target": masks, "mask_size": sizes}}
    ret_in = {"task_name": "TaskRetrieval", "task_input": {"text_features": text}}
    opt = torch.optim.AdamW([p for p in w.parameters() if p.requires_grad], lr=1e-3)
    seen = []
    for task in (vis_in, ret_in, vis_in, ret_in, vis_in):
        losses, _ = w(x, multi_task_input=task)
        loss = losses[task["task_name"]]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if task is vis_in:
            seen.append(float(loss))
    torch.cuda.synchronize()
    assert all(np.isfinite(seen)) and seen[-1] < seen[0], seen
