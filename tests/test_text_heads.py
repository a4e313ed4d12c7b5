"""The caption-driven heads: temporal grounding (``sf_grounding_loss``) and referring segmentation (``sf_dense_text_logits`` for its
evaluation output; ``sf_mask_loss`` / ``sf_dense_head_*`` for training) — against tests/text_heads_oracle.py, which
tools/make_golden_text_heads.py pins to the reference (fixture F17, tests/golden/f17_text_heads.npz: the reference's own tensors).

Kernel bounds.  The yardstick is the fp32 floor recorded in F17: the reference's operator sequence evaluated in fp32 against the same
sequence in fp64 on the same inputs, max-abs error over the tensor's max-abs, measured on the CPU by the generator — grounding
(loss, d pooler, d scalars, logits) 3.2e-7, 1.6e-7, 1.1e-7, 1.1e-7 on the fixture and 4.3e-7, 2.4e-7, 8.2e-8, 1.5e-7 at 8 x 16 x 768;
dense text logits 1.5e-7 / 1.8e-7 on the fixture rows, 3.2e-7 at 25 088 x 768 x 8, 1.0e-7 .. 3.3e-7 on the edge shapes.  A kernel is
allowed ``FLOOR_FACTOR`` (8, the constant of tests/test_spatial_head.py) times the floor of the same inputs — it adds a row's products
in another order than torch and uses the hardware exponential — and ``LOSS_TOL`` on the loss.

The referring head's fixture cases (``ra``, ``rb``) are one step away from the reference's forward as shipped: it hard-codes a 224-pixel
mask height and a 14 x 14 patch grid, and the generator runs its forward with exactly those two literals replaced by the fixture
config's 48 and 3 x 3 (a 224 / 14 x 14 case would not fit a fixture); everything else is the reference's code and tensors.

Through the dense projection (bf16 operands, fp32 accumulation) the bounds are those tests/test_spatial_head.py applies to the same
projection: relative L2 5e-2 / cosine 0.998 on gradients, relative L2 2e-2 on its forward output — here on the scaled similarities
``logits - logit_bias``, which are linear in the unit rows the projection produces.
"""
import os

import numpy as np
import pytest
import torch

from tests import spatial_head_oracle as S
from tests import text_heads_oracle as X
from tests.helpers import cosine, load_npz, maxabs, rel_l2, small_cfg
from tests.test_spatial_head import FLOOR_FACTOR, LOSS_TOL, f16_cfg, fp64_mask_loss, relmax
from tests.train_support import GRAD_COS, GRAD_REL_L2, SCALAR_REL, to_dev

T_FRAMES = 4
GROUNDING_NAMES = ("CharadesSTA", "QVHighlights", "TaCoS", "TVSum", "ActivityNetCaptions", "DiDeMo", "QuerYD", "TaskGrounding")
REFER_NAMES = ("MEVIS", "ReferYoutubeVOS", "RefCOCOPseudo", "TaskReferVOS")
LS, LB = float(np.float32(np.log(10.0))), -2.0        # the fp32 value the kernels read: the fp64 yardstick starts from the same number


@pytest.fixture(scope="module")
def f17(golden_dir):
    return load_npz(os.path.join(golden_dir, "f17_text_heads.npz"))


def seeded(f17, key, *shape):
    t = S.seeded_randn(int(f17[f"{key}_seed"]), *shape)
    assert abs(float(t.double().sum()) - float(f17[f"{key}_sum"])) < 1e-6, "RNG drift: seeded inputs differ from the fixture's"
    return t


def head_weights(f17):
    from streamformer_amd.init_weights import make_state_dict, state_dict_sha256
    cfg = f16_cfg()
    sd = make_state_dict(cfg, seed=int(f17["weights_seed"]))
    assert state_dict_sha256(sd) == str(f17["state_dict_sha256"]), "RNG drift: the seeded weights differ from the fixture's"
    D = cfg.hidden_size
    vals = (sd["head.attention.in_proj_weight"][2 * D:], sd["head.attention.in_proj_bias"][2 * D:], sd["head.attention.out_proj.weight"],
            sd["head.attention.out_proj.bias"], sd["head.layernorm.weight"], sd["head.layernorm.bias"], sd["head.mlp.fc1.weight"],
            sd["head.mlp.fc1.bias"], sd["head.mlp.fc2.weight"], sd["head.mlp.fc2.bias"])
    return {n: v.clone() for n, v in zip(S.PROJ_NAMES, vals)}, sd


def grounding_inputs(f17):
    labels = torch.from_numpy(f17["g_labels"])
    B, T = labels.shape
    D = f16_cfg().hidden_size
    return seeded(f17, "g_pooler", B, T, D), seeded(f17, "g_text", B, D), labels


def refer_inputs(f17, tag):
    cfg = f16_cfg()
    sizes = [tuple(int(v) for v in s) for s in f17[f"{tag}_mask_sizes"]]
    B, D = len(sizes), cfg.hidden_size
    lhs = seeded(f17, f"{tag}_lhs", B, T_FRAMES, cfg.num_patches, D)
    text = seeded(f17, f"{tag}_text", B, D)
    rank = int(f17[f"{tag}_rank"])
    text_all = torch.cat([S.seeded_randn(int(f17[f"{tag}_other_text_seed"]), B, D), text]) if rank else text
    masks = [torch.from_numpy(f17[f"{tag}_mask{i}"].astype(np.int64)) for i in range(B)]
    return cfg, lhs, text, text_all, rank, masks, sizes


def scalars(dtype=torch.float32):
    return torch.tensor(LS, dtype=dtype).requires_grad_(True), torch.tensor(LB, dtype=dtype).requires_grad_(True)


def fp64_grounding(pooler, text, labels):
    p = pooler.detach().cpu().double().requires_grad_(True)
    s, b = scalars(torch.float64)
    loss, logits = X.grounding_loss(p, text.cpu().double(), labels.cpu(), s, b)
    loss.backward()
    return loss.detach(), p.grad, torch.stack([s.grad, b.grad]), logits.detach()


def fp64_refer(cfg, lhs, proj, text_all, rank, masks, sizes):
    x = lhs.detach().double().requires_grad_(True)
    p = {k: v.detach().double().requires_grad_(True) for k, v in proj.items()}
    s, b = scalars(torch.float64)
    loss = X.refer_head_loss(x, p, cfg.layer_norm_eps, text_all.double(), rank, masks, sizes, cfg.image_size, s, b)
    loss.backward()
    return loss.detach(), x.grad, {k: v.grad for k, v in p.items()}, s.grad, b.grad


# ------------------------------------------------------------------------------------------------ CPU
def test_grounding_restatement_matches_reference_fixture(f17):
    pooler, text, labels = grounding_inputs(f17)
    assert bool((labels[0] == 0).all()) and bool((labels[1] == 1).all())
    pooler.requires_grad_(True)
    s, b = scalars()
    loss, logits = X.grounding_loss(pooler, text, labels, s, b)
    loss.backward()
    assert maxabs(loss.detach(), f17["g_loss"]) < 1e-5 and maxabs(logits.detach(), f17["g_logits"]) < 1e-5
    assert maxabs(pooler.grad, f17["g_d_pooler"]) < 1e-6
    assert maxabs(s.grad, f17["g_d_logit_scale"]) < 1e-6 and maxabs(b.grad, f17["g_d_logit_bias"]) < 1e-6


@pytest.mark.parametrize("tag", ["ra", "rb"])
def test_refer_restatement_matches_reference_fixture(f17, tag):
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, tag)
    p, _ = head_weights(f17)
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    lhs.requires_grad_(True)
    s, b = scalars()
    loss = X.refer_head_loss(lhs, p, cfg.layer_norm_eps, text_all, rank, masks, sizes, cfg.image_size, s, b)
    loss.backward()
    assert maxabs(loss.detach(), f17[f"{tag}_loss"]) < 1e-5
    assert maxabs(lhs.grad, f17[f"{tag}_d_lhs"]) < 1e-6
    assert maxabs(s.grad, f17[f"{tag}_d_logit_scale"]) < 1e-6 and maxabs(b.grad, f17[f"{tag}_d_logit_bias"]) < 1e-6
    for n in S.PROJ_NAMES:
        assert maxabs(p[n].grad, f17[f"{tag}_d_{n}"]) < 1e-6, n
    with torch.no_grad():        # the reference's evaluation branch keeps the first B columns of the gathered table
        ev = X.refer_head_logits(lhs.detach(), {k: v.detach() for k, v in p.items()}, cfg.layer_norm_eps, text_all[:len(masks)], s.detach(), b.detach())
    assert ev.shape == (len(masks), T_FRAMES, cfg.num_patches, len(masks)) and maxabs(ev, f17[f"{tag}_eval_logits"]) < 1e-5


@pytest.mark.parametrize("tag", ["ra", "rb"])
def test_refer_target_construction_equals_the_recorded_targets(f17, tag):
    from streamformer_amd.multitask import refer_mask_targets
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, tag)
    B = len(masks)
    assert (tag == "rb") == (rank == 1) and text_all.shape[0] == (rank + 1) * B
    got = refer_mask_targets(masks, rank, B)
    for i, (g, m) in enumerate(zip(got, masks)):
        want = torch.from_numpy(f17[f"{tag}_target{i}"].astype(np.int64))
        assert torch.equal(g, want) and torch.equal(X.refer_targets(masks, rank, B)[i], want)
        assert set(torch.unique(g).tolist()) <= {-1, rank * B + i} and int((g >= 0).sum()) == int((m == 1).sum()) > 0
        assert tuple(m.shape[-2:]) == (cfg.image_size, S.mask_width(cfg.image_size, sizes[i]))      # the mask width rule
    assert int((masks[2] == 1).sum()) < 0.02 * masks[2].numel()                                     # the clip with few positive pixels


def _wrapper(f17, tasks):
    import streamformer_amd as sa
    cfg = f16_cfg()
    _, sd = head_weights(f17)
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, tasks)
    w.timesformer.load_state_dict(sd)
    w.prepare_for_multi_tasks()
    return cfg, sd, w


def test_wrapper_builds_both_heads_for_every_reference_task_name(f17):
    """Fails on a tree without the feature (NotImplementedError for both task types)."""
    import streamformer_amd as sa
    from streamformer_amd.multitask import TimesformerTemporalGroundingHead, TimesformerVideoContrastiveCrossEntropySegmentationHead
    cfg = f16_cfg()
    for name in GROUNDING_NAMES:
        assert isinstance(sa.StreamformerForMultiTaskingSigLIP(cfg, {name: {}}).task_heads[name], TimesformerTemporalGroundingHead)
    for name in REFER_NAMES:
        assert isinstance(sa.StreamformerForMultiTaskingSigLIP(cfg, {name: {"label2id": {}}}).task_heads[name],
                          TimesformerVideoContrastiveCrossEntropySegmentationHead)
    cfg, sd, w = _wrapper(f17, {"TaskGrounding": {}, "TaskReferVOS": {"label2id": {}}})
    g, r = w.task_heads["TaskGrounding"], w.task_heads["TaskReferVOS"]
    assert [n for n, _ in g.named_parameters()] == [str(n) for n in f17["grounding_param_names"]]
    assert [p.requires_grad for _, p in g.named_parameters()] == [bool(v) for v in f17["grounding_param_requires_grad"]]
    assert [n for n, _ in r.named_parameters()] == [str(n) for n in f17["refer_param_names"]]
    assert [p.requires_grad for _, p in r.named_parameters()] == [bool(v) for v in f17["refer_param_requires_grad"]]
    p, _ = head_weights(f17)
    named = dict(r.named_parameters())
    for n in S.PROJ_NAMES:                       # deep copies of the pooling head's tensors (modeling:1940-1955), not views
        assert torch.equal(named[n].detach(), p[n]), n
    assert named["w_v.weight"].data_ptr() != w.timesformer.head.attention.in_proj_weight.data_ptr()
    assert named["head.probe"] is w.timesformer.head.probe
    names = [n for n, _ in w.named_parameters()]
    assert len(names) == len(set(names)) and "task_heads.TaskReferVOS.w_v.weight" in names and "task_heads.TaskReferVOS.head.probe" not in names
    fresh = sa.StreamformerForMultiTaskingSigLIP(cfg, {"TaskReferVOS": {"label2id": {}}}).task_heads["TaskReferVOS"]
    assert not hasattr(fresh, "w_v")             # as the reference: the projection is created by prepare_multi_task


def test_shipped_recipe_constructs_and_the_remaining_refusals_stay(f17):
    import streamformer_amd as sa
    cfg = f16_cfg()
    w = sa.StreamformerForMultiTaskingSigLIP(cfg, {"Kinetics": {"label2id": {}}, "TaskRetrieval": {}, "TaskGrounding": {},
                                                   "TaskLocalization": {"label2id": {}}, "TaskVIS": {"label2id": {}}})
    w.prepare_for_multi_tasks()
    assert len(w.task_heads) == 5
    for name in ("SSV2", "THUMOS14", "NoSuchTask"):
        with pytest.raises(NotImplementedError):
            sa.StreamformerForMultiTaskingSigLIP(cfg, {name: {"label2id": {}}})


def test_refusals_come_with_a_message(f17):
    """Shape and capacity errors are raised before anything is launched (no GPU needed)."""
    import ctypes
    import streamformer_amd._native as nat
    from streamformer_amd.heads import DenseTextLogits, GroundingHead
    from streamformer_amd.modeling import ModelOutput
    pooler, text, labels = grounding_inputs(f17)
    with pytest.raises(ValueError, match="text_features must be"):
        GroundingHead().loss(pooler, text[:2], labels)
    with pytest.raises(ValueError, match="text_features must be"):
        GroundingHead().loss(pooler, text[:, :64], labels)
    with pytest.raises(ValueError, match="labels must be"):
        GroundingHead().loss(pooler, text, labels[:, :5])
    with pytest.raises(ValueError, match="at most 64"):
        DenseTextLogits().forward(torch.zeros(16, 128), torch.ones(65, 128))
    with pytest.raises(ValueError, match="text_features must be"):
        DenseTextLogits().forward(torch.zeros(16, 128), torch.ones(4, 96))
    one = ctypes.c_void_p(256)
    assert nat.lib.sf_dense_text_logits(one, one, 16, 128, 65, one, one, one, None) == nat.SF_ERR_CAPACITY and b"captions" in nat.lib.sf_last_error()
    assert nat.lib.sf_dense_text_logits(one, one, 16, 130, 4, one, one, one, None) == nat.SF_ERR_INVALID and b"multiple of 4" in nat.lib.sf_last_error()
    assert nat.lib.sf_dense_text_logits(one, one, 16, 4096, 4, one, one, one, None) == nat.SF_ERR_CAPACITY and b"feature width" in nat.lib.sf_last_error()
    assert nat.lib.sf_dense_text_logits(one, one, 0, 128, 4, one, one, one, None) == nat.SF_ERR_INVALID
    assert nat.lib.sf_dense_text_logits(ctypes.c_void_p(260), one, 16, 128, 4, one, one, one, None) == nat.SF_ERR_INVALID and b"aligned" in nat.lib.sf_last_error()
    assert nat.lib.sf_grounding_loss(one, one, one, 2, 0, 128, one, one, one, None, None, None, one, 1 << 20, None) == nat.SF_ERR_INVALID
    assert nat.lib.sf_grounding_loss(one, one, one, 2, 8, 128, one, one, one, None, None, None, one, 16, None) == nat.SF_ERR_WORKSPACE
    assert b"workspace" in nat.lib.sf_last_error()
    cfg, sd, w = _wrapper(f17, {"TaskReferVOS": {"label2id": {}}, "TaskGrounding": {}})
    lhs = torch.zeros(3, T_FRAMES, cfg.num_patches, cfg.hidden_size)
    with pytest.raises(ValueError, match="text_features must be"):
        w.task_heads["TaskReferVOS"](ModelOutput(last_hidden_state=lhs), {"text_features": torch.ones(2, cfg.hidden_size)})
    with pytest.raises(ValueError, match="labels must be"):
        w.task_heads["TaskGrounding"](ModelOutput(pooler_output=pooler), {"text_features": text, "label": labels.t()})


# ------------------------------------------------------------------------------------------------ GPU
# local: as in test_spatial_head.py, a missing GPU skips
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def run_grounding(pooler, text, labels):
    from streamformer_amd.heads import GroundingHead
    out = GroundingHead(LS, LB).loss(pooler.cuda(), text.cuda(), labels.cuda(), return_logits=True)
    torch.cuda.synchronize()
    return out


def check_grounding(pooler, text, labels, floor, what):
    loss, gp, gs, logits = run_grounding(pooler, text, labels)
    want, wgp, wgs, wz = fp64_grounding(pooler, text, labels)
    e = (abs(float(loss) - float(want)), relmax(gp, wgp), relmax(gs, wgs), relmax(logits, wz))
    print(f"{what}: loss {float(loss):.6f} err {e[0]:.2e} | d pooler {e[1]:.2e} (floor {floor[1]:.2e}) | d scalars {e[2]:.2e} (floor {floor[2]:.2e})"
          f" | logits {e[3]:.2e} (floor {floor[3]:.2e})")
    assert e[0] < LOSS_TOL, (what, e)
    for i in (1, 2, 3):
        assert e[i] <= FLOOR_FACTOR * floor[i], (what, i, e[i], floor[i])
    return loss, gp, gs, logits


@pytest.mark.gpu
def test_grounding_loss_kernel_vs_fp64(f17):
    _gpu()
    pooler, text, labels = grounding_inputs(f17)
    loss, gp, gs, logits = check_grounding(pooler, text, labels, f17["g_floor"], "F17 g")
    from streamformer_amd.heads import GroundingHead
    l2, gp2, gs2 = GroundingHead(LS, LB).loss(pooler.cuda(), text.cuda(), labels.cuda(), need_grad=False)       # NULL gradient / logits pointers
    assert gp2 is None and gs2 is None and torch.equal(l2, loss)
    assert torch.equal(GroundingHead(LS, LB).logits(pooler.cuda(), text.cuda()), logits)
    check_grounding(*X.bench_grounding_inputs(), f17["bench_g_floor"], "8 x 16 x 768")
    # labels are numbers: anything but 0 is used as given (the reference's masked_fill), e.g. soft or signed targets
    odd = torch.tensor([[0.0, 1.0, -1.0, 2.0, 0.5, 0.0, 1.0, -0.25]] * 3)
    check_grounding(pooler, text, odd, f17["g_floor"], "numeric labels")


def run_dense(x, text):
    from streamformer_amd.heads import DenseTextLogits
    out = DenseTextLogits(LS, LB).forward(x.cuda(), text.cuda())
    torch.cuda.synchronize()
    return out


def check_dense(x, text, floor, what):
    got = run_dense(x, text)
    with torch.no_grad():
        want = X.dense_text_logits(x.double(), text.double(), torch.tensor(LS, dtype=torch.float64), torch.tensor(LB, dtype=torch.float64))
    e = relmax(got, want)
    print(f"dense text logits {what}: {tuple(got.shape)} err {e:.2e} (floor {floor:.2e})")
    assert got.shape == want.shape and e <= FLOOR_FACTOR * floor, (what, e, floor)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ra", "rb"])
def test_dense_text_logits_kernel_vs_fp64_on_the_fixture_rows(f17, tag):
    _gpu()
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, tag)
    p, _ = head_weights(f17)
    dense = S.dense_projection(lhs.double(), {k: v.double() for k, v in p.items()}, cfg.layer_norm_eps).float()
    got = check_dense(dense, text, float(f17[f"{tag}_floor"][3]), f"F17 {tag}")
    assert got.shape == (3, T_FRAMES, cfg.num_patches, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ra", "rb"])
def test_mask_loss_kernel_on_the_caption_tables_vs_fp64(f17, tag):
    """``sf_mask_loss`` as the referring head feeds it — one gathered caption table for every clip, one positive class per clip — at the
    fp32 floor of the same inputs (``r*_floor`` loss / d dense / d scalars)."""
    _gpu()
    from streamformer_amd.heads import MaskLossHead
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, tag)
    p, _ = head_weights(f17)
    dense = S.dense_projection(lhs.double(), {k: v.double() for k, v in p.items()}, cfg.layer_norm_eps).float()
    tables, targets = [X.refer_table(text_all)] * len(masks), X.refer_targets(masks, rank, len(masks))
    loss, gx, gs = MaskLossHead(LS, LB).loss(dense.cuda(), [t.cuda() for t in tables], [t.cuda() for t in targets])
    torch.cuda.synchronize()
    want, wgx, wgs = fp64_mask_loss(dense, tables, targets, ls=LS, lb=LB)
    floor = f17[f"{tag}_floor"]
    e = (abs(float(loss) - float(want)), relmax(gx, wgx), relmax(gs, wgs))
    print(f"mask loss on the caption table, F17 {tag}: loss err {e[0]:.2e} | d dense {e[1]:.2e} (floor {floor[1]:.2e}) | d scalars {e[2]:.2e} (floor {floor[2]:.2e})")
    assert e[0] < LOSS_TOL and e[1] <= FLOOR_FACTOR * floor[1] and e[2] <= FLOOR_FACTOR * floor[2], (tag, e, floor)


@pytest.mark.gpu
def test_dense_text_logits_kernel_vs_fp64_at_the_benchmark_shape(f17):
    _gpu()
    check_dense(*X.bench_dense_inputs(), float(f17["bench_t_floor"][0]), "25088 x 768 x 8")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(X.EDGE_DENSE_SHAPES))
def test_dense_text_logits_edge_shapes(f17, name):
    _gpu()
    seed, M, D, n = X.EDGE_DENSE_SHAPES[name]
    x, text = X.bench_dense_inputs(seed, M, D, n)
    check_dense(x, text, float(f17[f"edge_t_floor_{name}"][0]), f"{name} {M} x {D} x {n}")
    guard = torch.full((M + 8, n), float("nan"))          # nothing is written past the last row
    from streamformer_amd.heads import DenseTextLogits
    import streamformer_amd._native as nat
    out, xd, td = guard.cuda(), x.cuda(), text.cuda()
    one = torch.tensor([LS, LB], device="cuda")
    nat.check(nat.lib.sf_dense_text_logits(xd.data_ptr(), td.data_ptr(), M, D, n, one[0:].data_ptr(), one[1:].data_ptr(), out.data_ptr(),
                                           nat.current_stream_handle(out.device)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[M:]).all()) and torch.equal(out[:M], DenseTextLogits(LS, LB).forward(xd, td))


@pytest.mark.gpu
def test_both_kernels_are_bit_reproducible(f17):
    _gpu()
    pooler, text, labels = X.bench_grounding_inputs()
    x, t = X.bench_dense_inputs(M=4001, n=8)
    x2, t2 = X.bench_dense_inputs(*X.EDGE_DENSE_SHAPES["n64"])
    first = run_grounding(pooler, text, labels) + (run_dense(x, t), run_dense(x2, t2))
    for _ in range(9):
        again = run_grounding(pooler, text, labels) + (run_dense(x, t), run_dense(x2, t2))
        for a, b in zip(first, again):
            assert torch.equal(a, b)


def _grounding_oracle(*a, **kw):
    """oracle.train_oracle.OracleTrainer with the grounding restatement as one more loss kind."""
    from oracle import streamformer_oracle as O
    from oracle import train_oracle as TO

    class Oracle(TO.OracleTrainer):
        def loss(self, task, pixels, task_input, **kws):
            if task_input["kind"] != "grounding":
                return super().loss(task, pixels, task_input, **kws)
            out = O.forward_graph(self.sd, self.cfg, pixels)
            h = self.heads[task]
            return X.grounding_loss(out["pooler_output"], task_input["text"], task_input["labels"], h["logit_scale"], h["logit_bias"])[0]
    return Oracle(*a, **kw)


def _train_setup(lr=1e-3, wd=0.05):
    from streamformer_amd.init_weights import make_state_dict
    from streamformer_amd.training import StreamformerTrainer
    cfg = small_cfg(num_frames=8, add_lora_spatial=True)
    sd = make_state_dict(cfg, seed=8, lora=True)
    tr = StreamformerTrainer(cfg, sd, ["grounding", "retrieval"], freeze_spatial=True, device=torch.device("cuda:0"), lr=lr, weight_decay=wd)
    orc = _grounding_oracle(sd, cfg, ["grounding", "retrieval"], freeze_spatial=True, lr=lr, weight_decay=wd)
    B, T, D = 2, 8, cfg.hidden_size
    x = S.seeded_randn(1780, B, T, 3, cfg.image_size, cfg.image_size)
    g = torch.Generator().manual_seed(1783)
    ground = {"kind": "grounding", "text": S.seeded_randn(1781, B, D), "labels": torch.randint(0, 2, (B, T), generator=g)}
    retr = {"kind": "retrieval", "text": S.seeded_randn(1782, B, D)}
    return cfg, sd, tr, orc, x, ground, retr


@pytest.mark.gpu
def test_grounding_through_the_wrapper_and_the_trainer_vs_oracle_autograd():
    """loss.backward() through StreamformerForMultiTaskingSigLIP fills the encoder's .grad with the oracle's autograd gradients of the
    grounding restatement, and StreamformerTrainer.micro_step(kind="grounding") accumulates the same gradients."""
    dev = _gpu()
    import streamformer_amd as sa
    cfg, sd, tr, orc, x, ground, retr = _train_setup()
    model = sa.StreamformerForMultiTaskingSigLIP(cfg, {"TaskGrounding": {}, "TaskRetrieval": {}})
    model.timesformer.load_state_dict(sd)
    model.prepare_for_multi_tasks()
    model.frozen_spatial()
    model.cuda().train()
    losses, outs = model(x.to(dev), multi_task_input={"task_name": "TaskGrounding",
                                                      "task_input": {"text_features": ground["text"].to(dev), "label": ground["labels"].to(dev)}})
    losses["TaskGrounding"].backward()
    torch.cuda.synchronize()
    want_loss = orc.loss("grounding", x, ground)
    want_loss.backward()
    og = orc.grads()
    assert abs(float(losses["TaskGrounding"]) - float(want_loss)) < 2e-2 * abs(float(want_loss))
    assert outs["TaskGrounding"].shape == (2, 8)
    # update_freq = 2: the first micro-step accumulates half the gradient and leaves the optimizer alone
    got_loss = tr.micro_step("grounding", x.to(dev), to_dev(ground, dev), update_freq=2)
    torch.cuda.synchronize()
    assert abs(float(got_loss) - float(losses["TaskGrounding"])) < 1e-3 * abs(float(got_loss)) + 1e-5
    named = dict(model.timesformer.named_parameters())
    checked, worst = 0, (0.0, 1.0)
    for n in tr.parameter_names(trainable_only=True):
        if n not in named:
            continue
        p, want = named[n], og[n]
        assert p.requires_grad and p.grad is not None, n
        if want.numel() == 1 or float(want.abs().max()) < 1e-6:
            continue
        r, c = rel_l2(p.grad, want), cosine(p.grad, want)
        rt, ct = rel_l2(tr.grad(n) * 2, p.grad), cosine(tr.grad(n), p.grad)
        worst = (max(worst[0], r, rt), min(worst[1], c, ct))
        assert r < GRAD_REL_L2 and c > GRAD_COS, (n, "wrapper vs oracle", r, c)
        assert rt < GRAD_REL_L2 and ct > GRAD_COS, (n, "trainer vs wrapper", rt, ct)
        checked += 1
    print(f"grounding: {checked} tensors, worst rel-L2 {worst[0]:.3e}, lowest cosine {worst[1]:.6f}")
    assert checked > 20
    head = model.task_heads["TaskGrounding"]
    for k, t in (("logit_scale", head.logit_scale), ("logit_bias", head.logit_bias)):
        w, got_w, got_t = float(og[f"task_heads.grounding.{k}"]), float(t.grad), 2 * float(tr.grad(f"task_heads.grounding.{k}"))
        print(f"grounding d {k}: wrapper {got_w:.6f} trainer x 2 {got_t:.6f} oracle {w:.6f}")
        assert abs(got_w - w) < SCALAR_REL * abs(w), k        # bf16 encoder against the fp32 oracle: the bound of test_train_widths.py
        # the same kernels on the same pooled vectors: only the summation of the two paths' forwards may differ, never a factor
        assert abs(got_t - got_w) < 1e-3 * abs(got_w), (k, "update_freq scaling")
    model.eval()
    with torch.no_grad():
        ev = model(x.to(dev), multi_task_input={"task_name": "TaskGrounding", "task_input": {"text_features": ground["text"].to(dev)}})
    assert ev["TaskGrounding"].shape == (2, 8) and rel_l2(ev["TaskGrounding"], outs["TaskGrounding"]) < 2e-2


@pytest.mark.gpu
def test_three_adamw_steps_alternating_grounding_and_retrieval_track_the_oracle():
    dev = _gpu()
    cfg, sd, tr, orc, x, ground, retr = _train_setup()
    got, want = [], []
    for task, ti in (("grounding", ground), ("retrieval", retr), ("grounding", ground)):
        want_loss = orc.loss(task, x, ti)
        want_loss.backward()
        torch.nn.utils.clip_grad_norm_(list(orc.named.values()), 1.0)
        orc.opt.step()
        orc.opt.zero_grad(set_to_none=True)
        want.append(float(want_loss.detach()))
        got.append(float(tr.micro_step(task, x.to(dev), to_dev(ti, dev), lr=1e-3, weight_decay=0.05, clip_grad=1.0)))
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print("grounding / retrieval / grounding losses (trainer, oracle):", list(zip(got, want)))
    assert max(rel) < 3e-2, list(zip(got, want))


def _patch_world(monkeypatch, rank, other):
    """World 2 as seen from `rank` 1: the other rank's captions come first in the gathered table."""
    import streamformer_amd.parallel as par
    monkeypatch.setattr(par, "world", lambda group=None: (rank, 2))
    monkeypatch.setattr(par, "all_gather_rows", lambda t, group=None, at_world_1=False: torch.cat([other.to(t.device), t]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ra", "rb"])
def test_refer_head_training_vs_fp64_restatement(f17, tag, monkeypatch):
    dev = _gpu()
    from streamformer_amd.modeling import ModelOutput
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, tag)
    if rank:
        _patch_world(monkeypatch, rank, text_all[:len(masks)])
    _, _, w = _wrapper(f17, {"TaskReferVOS": {"label2id": {}}})
    head = w.cuda().train().task_heads["TaskReferVOS"]
    x = lhs.to(dev).requires_grad_(True)
    loss, _ = head(ModelOutput(last_hidden_state=x), {"text_features": text.to(dev), "mask_target": masks, "mask_size": sizes})
    loss.backward()
    torch.cuda.synchronize()
    p, _ = head_weights(f17)
    want, wx, wp, ws, wb = fp64_refer(cfg, lhs, p, text_all, rank, masks, sizes)
    named = dict(head.named_parameters())
    print(f"refer {tag}: loss {float(loss):.6f} want {float(want):.6f}; d lhs rel-L2 {rel_l2(x.grad, wx):.2e}; d logit_scale {float(named['logit_scale'].grad):.5f} "
          f"want {float(ws):.5f}")
    assert abs(float(loss) - float(want)) < 2e-2 * abs(float(want)) + 1e-2
    for name, got, ref in [("d last_hidden_state", x.grad, wx)] + [(n, named[n].grad, wp[n]) for n in S.PROJ_NAMES]:
        r, c = rel_l2(got, ref), cosine(got, ref)
        assert r <= 5e-2 and c >= 0.998, (name, r, c)
    assert abs(float(named["logit_scale"].grad) - float(ws)) < 5e-2 * abs(float(ws))
    # d logit_bias is mathematically zero (a shift of every logit of a pixel cancels in the softmax)
    assert abs(float(named["logit_bias"].grad)) < 1e-5 and abs(float(wb)) < 1e-12
    assert head._proj._ws is None                # the backward handed the projection workspace back


@pytest.mark.gpu
def test_refer_head_eval_logits_and_released_workspace(f17):
    dev = _gpu()
    from streamformer_amd.heads import DenseHeadProjection, DenseTextLogits
    from streamformer_amd.modeling import ModelOutput
    cfg, lhs, text, text_all, rank, masks, sizes = refer_inputs(f17, "ra")
    _, _, w = _wrapper(f17, {"TaskReferVOS": {"label2id": {}}})
    head = w.cuda().eval().task_heads["TaskReferVOS"]
    got = head(ModelOutput(last_hidden_state=lhs.to(dev)), {"text_features": text.to(dev)})
    torch.cuda.synchronize()
    assert got.shape == (3, T_FRAMES, cfg.num_patches, 3) and not got.requires_grad
    assert head._proj._ws is None and head._proj._params is None, "the eval forward must release the projection's saved activations"
    p, _ = head_weights(f17)
    with torch.no_grad():
        want = X.refer_head_logits(lhs.double(), {k: v.double() for k, v in p.items()}, cfg.layer_norm_eps, text.double(),
                                   torch.tensor(LS, dtype=torch.float64), torch.tensor(LB, dtype=torch.float64))
    r = rel_l2(got - LB, want - LB)
    print(f"refer eval: scaled similarities rel-L2 {r:.2e}, logits max-abs {maxabs(got, want):.2e}")
    assert r < 2e-2
    proj = DenseHeadProjection(cfg.layer_norm_eps)           # the head is exactly projection -> sf_dense_text_logits
    dense = proj.forward(lhs.to(dev), [p[n].to(dev) for n in S.PROJ_NAMES])
    assert torch.equal(got, DenseTextLogits(head.logit_scale, head.logit_bias).forward(dense, text.to(dev)))
    with pytest.raises(ValueError, match="at most 64"):
        DenseTextLogits().forward(dense, torch.ones(65, cfg.hidden_size, device=dev))
