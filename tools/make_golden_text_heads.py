"""Generate tests/golden/f17_text_heads.npz by running the REFERENCE caption-driven heads, and pin tests/text_heads_oracle.py against them.

Build machine only (needs the reference checkout beside the repository, like oracle/make_golden.py); CPU only:

    python tools/make_golden_text_heads.py            # writes the fixture, asserts restatement == reference
    python tools/make_golden_text_heads.py --floor    # additionally measures the fp32 floors of the benchmark-sized shapes

The reference classes are imported at run time; what is stored is data.  Both heads want a tokenizer and a text encoder: they get
stubs that return fixed feature rows (``outputs[1]``), and a one-process gloo group answers ``dist.get_world_size()`` / ``get_rank()``.

F17 cases (the F16 config: image_size 48 -> 3 x 3 patches, hidden_size 128, intermediate_size 64, 4 frames; seeded weights, SHA recorded):
  g   TimesformerTemporalGroundingHead: 3 clips x 8 frames, label rows all-zero / all-one / mixed
  ra  TimesformerVideoContrastiveCrossEntropySegmentationHead: 3 clips x 4 frames, mask_size (96, 120) -> 48 x 60, (64, 40) -> 48 x 30 and
      (48, 48); the third mask has few positive pixels; masks also hold values other than 0 / 1 (ignored like 0)
  rb  the same head with a gathered table larger than the local batch: world 2, rank 1 (``dist.get_rank`` / ``all_gather`` patched),
      so clip i's target is 3 + i; its ``eval_logits`` are against the first 3 rows of the gathered table (rank 0's captions), which
      is what the reference's evaluation branch returns on rank 1
Per case: inputs as seeds + checksums (masks as arrays), the reference's loss, logits and gradients, the targets, parameter name lists.
``*_floor``: the reference's operator sequence evaluated in fp32 against the same sequence in fp64 on the same inputs, max-abs error
over the tensor's max-abs (the loss: absolute) — the yardstick of the kernels' bounds in tests/test_text_heads.py.
  g_floor / bench_g_floor   (loss, d pooler, d scalars, logits)
  r*_floor                  (loss, d dense, d scalars, eval logits);  bench_t_floor / edge_t_floor_<name>: (logits,)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "f17_text_heads.npz")

from oracle.make_golden import build_ref, import_reference, maxabs, small_cfg  # noqa: E402
from streamformer_amd.init_weights import make_state_dict, state_dict_sha256  # noqa: E402
from tests import spatial_head_oracle as S  # noqa: E402
from tests import text_heads_oracle as X  # noqa: E402

SEED_WEIGHTS = 16            # the F16 weights
T_FRAMES = 4


class StubTokenizer:
    def __call__(self, captions, **kw):
        return types.SimpleNamespace(to=lambda device: {"n": len(captions)})


class StubTextEncoder(torch.nn.Module):
    """``outputs[1]`` = fixed feature rows, one per caption."""

    def __init__(self, rows):
        super().__init__()
        self.rows = rows

    def forward(self, n):
        assert n == self.rows.shape[0]
        return (None, self.rows)


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def scalars():
    return torch.nn.Parameter(torch.log(torch.tensor(10.0))), torch.nn.Parameter(torch.tensor(-2.0))


def grounding_floor(pooler, text, labels):
    out = []
    for dt in (torch.float32, torch.float64):
        p = pooler.detach().to(dt).requires_grad_(True)
        s, b = torch.log(torch.tensor(10.0)).to(dt).requires_grad_(True), torch.tensor(-2.0).to(dt).requires_grad_(True)
        loss, logits = X.grounding_loss(p, text.to(dt), labels, s, b)
        loss.backward()
        out.append((loss.detach(), p.grad, torch.stack([s.grad, b.grad]), logits.detach()))
    (l32, g32, s32, z32), (l64, g64, s64, z64) = out
    return (float((l32.double() - l64).abs()), relmax(g32, g64), relmax(s32, s64), relmax(z32, z64))


def mask_floor(dense, tables, targets, ls, lb):
    """As tools/make_golden_spatial_head.py: fp32 operator sequence vs fp64, (loss abs error, d dense, d scalars relative max-abs)."""
    out = []
    for dt in (torch.float32, torch.float64):
        x = dense.detach().to(dt).requires_grad_(True)
        s, b = ls.detach().to(dt).requires_grad_(True), lb.detach().to(dt).requires_grad_(True)
        loss = S.mask_loss(x, [t.to(dt) for t in tables], targets, s, b)
        loss.backward()
        out.append((loss.detach(), x.grad, torch.stack([s.grad, b.grad])))
    (l32, g32, s32), (l64, g64, s64) = out
    return (float((l32.double() - l64).abs()), relmax(g32, g64), relmax(s32, s64))


def logits_floor(x, text):
    s, b = torch.log(torch.tensor(10.0)), torch.tensor(-2.0)
    with torch.no_grad():
        return relmax(X.dense_text_logits(x, text, s, b), X.dense_text_logits(x.double(), text.double(), s.double(), b.double()))


def run_grounding(M, cfg, out):
    B, T, D = 3, 8, cfg.hidden_size
    pooler = S.seeded_randn(1701, B, T, D).requires_grad_(True)
    text = S.seeded_randn(1702, B, D)
    labels = torch.tensor([[0] * T, [1] * T, [0, 0, 1, 1, 1, 0, 1, 0]])
    head = M.TimesformerTemporalGroundingHead(cfg)
    ls, lb = scalars()
    head.prepare_multi_task(StubTextEncoder(text), StubTokenizer(), ls, lb, None)
    head.train()
    loss, logits = head(types.SimpleNamespace(pooler_output=pooler), {"caption": ["c"] * B, "label": labels})
    loss.backward()
    p2 = pooler.detach().clone().requires_grad_(True)
    s2, b2 = head.logit_scale.detach().clone().requires_grad_(True), head.logit_bias.detach().clone().requires_grad_(True)
    loss2, logits2 = X.grounding_loss(p2, text, labels, s2, b2)
    loss2.backward()
    assert maxabs(loss2, loss) <= 1e-6 and maxabs(logits2, logits) <= 1e-6 and maxabs(p2.grad, pooler.grad) <= 1e-7
    assert maxabs(s2.grad, head.logit_scale.grad) <= 1e-6 and maxabs(b2.grad, head.logit_bias.grad) <= 1e-6
    fl = grounding_floor(pooler, text, labels)
    print(f"  g: loss {float(loss):.6f}  restatement == reference;  fp32 floor: loss {fl[0]:.2e}  d pooler {fl[1]:.2e}  d scalars {fl[2]:.2e}  logits {fl[3]:.2e}")
    out.update({"g_pooler_seed": np.array(1701), "g_pooler_sum": np.array(float(pooler.detach().double().sum())), "g_text_seed": np.array(1702),
                "g_text_sum": np.array(float(text.double().sum())), "g_labels": labels.numpy(), "g_loss": loss.detach().numpy(),
                "g_logits": logits.detach().numpy(), "g_d_pooler": pooler.grad.numpy(), "g_d_logit_scale": head.logit_scale.grad.numpy(),
                "g_d_logit_bias": head.logit_bias.grad.numpy(), "g_floor": np.array(fl, dtype=np.float64),
                "grounding_param_names": np.array([n for n, _ in head.named_parameters() if not n.startswith("text_encoder.")]),
                "grounding_param_requires_grad": np.array([p.requires_grad for n, p in head.named_parameters() if not n.startswith("text_encoder.")])})


def run_refer(tag, M, ref_models, cfg, masks, sizes, lhs_seed, text_seed, out, other_text_seed=None):
    import torch.distributed as dist
    B, D = len(masks), cfg.hidden_size
    sd = make_state_dict(cfg, seed=SEED_WEIGHTS)
    enc = build_ref(ref_models, cfg, sd)
    text = S.seeded_randn(text_seed, B, D)
    head = M.TimesformerVideoContrastiveCrossEntropySegmentationHead(enc.config, {}, enc.head)
    ls, lb = scalars()
    head.prepare_multi_task(StubTextEncoder(text), StubTokenizer(), ls, lb, enc)
    rank, text_all = 0, text
    saved = (dist.get_rank, dist.all_gather)
    if other_text_seed is not None:           # world 2, this process is rank 1: rank 0's captions come first in the gathered table
        other = S.seeded_randn(other_text_seed, B, D)
        rank, text_all = 1, torch.cat([other, text])
        head.world_size = 2

        def fake_gather(tensor_list, tensor, *a, **k):
            tensor_list[0].copy_(other)
            tensor_list[1].copy_(tensor)
        dist.get_rank = lambda *a, **k: 1
        dist.all_gather = fake_gather
    try:
        lhs = S.seeded_randn(lhs_seed, B, T_FRAMES, cfg.num_patches, D).requires_grad_(True)
        ti = {"caption": ["c"] * B, "mask_target": masks, "mask_size": sizes}
        if cfg.image_size == 224 and cfg.num_patches == 196:
            head.train()
            loss, _ = head(types.SimpleNamespace(last_hidden_state=lhs), ti)
        else:
            # the reference hard-codes new_h = 224 and a 14 x 14 grid (modeling:2026-2030); at the fixture's 48-pixel / 3 x 3 config the
            # same forward is run with those two literals replaced, nothing else: the source of forward() is re-bound with the constants
            # of this config
            import inspect
            import textwrap
            src = textwrap.dedent(inspect.getsource(type(head).forward))
            assert "patch_size = 14" in src and "new_h = 224" in src
            P = int(round(cfg.num_patches ** 0.5))
            src = src.replace("patch_size = 14", f"patch_size = {P}").replace("new_h = 224", f"new_h = {cfg.image_size}")
            ns = dict(vars(M))
            exec(compile(src, "<reference forward at the fixture's geometry>", "exec"), ns)
            fwd = ns["forward"]
            head.train()
            loss, _ = fwd(head, types.SimpleNamespace(last_hidden_state=lhs), ti)
            head.eval()
            with torch.no_grad():
                ev = fwd(head, types.SimpleNamespace(last_hidden_state=lhs.detach()), ti)
            head.train()
        loss.backward()
        if cfg.image_size == 224 and cfg.num_patches == 196:
            head.eval()
            with torch.no_grad():
                ev = head(types.SimpleNamespace(last_hidden_state=lhs.detach()), ti)
            head.train()
    finally:
        dist.get_rank, dist.all_gather = saved
    named = dict(head.named_parameters())
    # restatement
    p = {n: named[n].detach().clone().requires_grad_(True) for n in S.PROJ_NAMES}
    lhs2 = lhs.detach().clone().requires_grad_(True)
    s2, b2 = named["logit_scale"].detach().clone().requires_grad_(True), named["logit_bias"].detach().clone().requires_grad_(True)
    loss2 = X.refer_head_loss(lhs2, p, cfg.layer_norm_eps, text_all, rank, masks, sizes, cfg.image_size, s2, b2)
    loss2.backward()
    assert maxabs(loss2, loss) <= 1e-6, (tag, float(loss), float(loss2))
    assert maxabs(lhs2.grad, lhs.grad) <= 1e-7, (tag, maxabs(lhs2.grad, lhs.grad))
    assert maxabs(s2.grad, named["logit_scale"].grad) <= 1e-6 and maxabs(b2.grad, named["logit_bias"].grad) <= 1e-6, tag
    for n in S.PROJ_NAMES:
        assert named[n].grad is not None and float(named[n].grad.abs().max()) > 0, (tag, n, "the reference trains this tensor")
        assert maxabs(p[n].grad, named[n].grad) <= 1e-6, (tag, n, maxabs(p[n].grad, named[n].grad))
    with torch.no_grad():
        pd = {n: named[n].detach() for n in S.PROJ_NAMES}
        # the reference's evaluation branch keeps the FIRST B columns of the gathered table (:2018): the local captions at rank 0 / world 1,
        # rank 0's captions on every other rank.  The recorded tensor is the reference's; the head here always answers for the local captions.
        ev2 = X.refer_head_logits(lhs.detach(), pd, cfg.layer_norm_eps, text_all[:B], named["logit_scale"].detach(), named["logit_bias"].detach())
        assert tuple(ev.shape) == (B, T_FRAMES, cfg.num_patches, B) and maxabs(ev2, ev) <= 2e-6, (tag, tuple(ev.shape), maxabs(ev2, ev))
        dense = S.dense_projection(lhs.detach(), pd, cfg.layer_norm_eps)
    targets = X.refer_targets(masks, rank, B)
    fl = mask_floor(dense, [X.refer_table(text_all)] * B, targets, named["logit_scale"], named["logit_bias"]) + (logits_floor(dense, text),)
    print(f"  {tag}: loss {float(loss):.6f}  restatement == reference;  fp32 floor: loss {fl[0]:.2e}  d dense {fl[1]:.2e}  d scalars {fl[2]:.2e}  eval logits {fl[3]:.2e}")
    out[f"{tag}_lhs_seed"] = np.array(lhs_seed)
    out[f"{tag}_lhs_sum"] = np.array(float(lhs.detach().double().sum()))
    out[f"{tag}_text_seed"] = np.array(text_seed)
    out[f"{tag}_text_sum"] = np.array(float(text.double().sum()))
    out[f"{tag}_rank"] = np.array(rank)
    if other_text_seed is not None:
        out[f"{tag}_other_text_seed"] = np.array(other_text_seed)
    out[f"{tag}_mask_sizes"] = np.array(sizes, dtype=np.int64)
    for i, m in enumerate(masks):
        out[f"{tag}_mask{i}"] = m.numpy().astype(np.uint8)
        out[f"{tag}_target{i}"] = targets[i].numpy().astype(np.int8)
    out[f"{tag}_loss"] = loss.detach().numpy()
    out[f"{tag}_eval_logits"] = ev.numpy()
    out[f"{tag}_d_lhs"] = lhs.grad.numpy()
    out[f"{tag}_d_logit_scale"] = named["logit_scale"].grad.numpy()
    out[f"{tag}_d_logit_bias"] = named["logit_bias"].grad.numpy()
    for n in S.PROJ_NAMES:
        out[f"{tag}_d_{n}"] = named[n].grad.numpy()
    out[f"{tag}_floor"] = np.array(fl, dtype=np.float64)
    return head, sd


def sparse_mask(seed, T, H, W, cells=4):
    """A mask with few positive pixels: a handful of isolated pixels per frame."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(T, H, W, dtype=torch.long)
    for t in range(T):
        ys, xs = torch.randint(0, H, (cells,), generator=g), torch.randint(0, W, (cells,), generator=g)
        m[t, ys, xs] = 1
    return m


def main():
    import torch.distributed as dist
    ref_models = import_reference()
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29581", rank=0, world_size=1)
    import models.modeling_timesformer_siglip as M
    cfg = small_cfg(intermediate_size=64, num_frames=T_FRAMES)
    H = cfg.image_size
    out = {}
    print("F17: temporal grounding head / referring segmentation head against the reference")
    run_grounding(M, cfg, out)
    sizes = [(96, 120), (64, 40), (48, 48)]
    widths = [S.mask_width(H, s) for s in sizes]
    assert widths == [60, 30, 48]
    masks = [S.blocky_mask(1710, T_FRAMES, H, 60, [0, 1, 1, 2]), S.blocky_mask(1711, T_FRAMES, H, 30, [0, 1, 3]), sparse_mask(1712, T_FRAMES, H, 48)]
    head, sd = run_refer("ra", M, ref_models, cfg, masks, sizes, 1713, 1714, out)
    keep = [(n, p) for n, p in head.named_parameters() if not n.startswith("text_encoder.")]
    out["refer_param_names"] = np.array([n for n, _ in keep])
    out["refer_param_requires_grad"] = np.array([p.requires_grad for _, p in keep])
    out["state_dict_sha256"] = np.array(state_dict_sha256(sd))
    out["weights_seed"] = np.array(SEED_WEIGHTS)
    masks = [S.blocky_mask(1720, T_FRAMES, H, 60, [0, 1]), S.blocky_mask(1721, T_FRAMES, H, 30, [0, 0, 1, 2]), sparse_mask(1722, T_FRAMES, H, 48, cells=9)]
    run_refer("rb", M, ref_models, cfg, masks, sizes, 1723, 1724, out, other_text_seed=1725)
    # fp32 floors of the dense text logits on the edge shapes of the GPU tests
    for name, (seed, Mr, D, n) in X.EDGE_DENSE_SHAPES.items():
        x, t = X.bench_dense_inputs(seed, Mr, D, n)
        out[f"edge_t_floor_{name}"] = np.array([logits_floor(x, t)], dtype=np.float64)
        print(f"  dense text logits {name} ({Mr} x {D} x {n}): fp32 floor {float(out[f'edge_t_floor_{name}'][0]):.2e}")
    if "--floor" in sys.argv:
        out["bench_g_floor"] = np.array(grounding_floor(*X.bench_grounding_inputs()), dtype=np.float64)
        out["bench_t_floor"] = np.array([logits_floor(*X.bench_dense_inputs())], dtype=np.float64)
        print(f"  benchmark shapes: grounding 8 x 16 x 768 floor {out['bench_g_floor']};  dense text logits 25088 x 768 x 8 floor {out['bench_t_floor']}")
    elif os.path.exists(OUT):
        old = np.load(OUT)
        for k in ("bench_g_floor", "bench_t_floor"):
            if k in old:
                out[k] = old[k]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
