"""Generate tests/golden/f16_vis_head.npz by running the REFERENCE heads, and pin tests/spatial_head_oracle.py against them.

Build machine only (needs the reference checkout beside the repository, like oracle/make_golden.py):

    python tools/make_golden_spatial_head.py            # writes the fixture, asserts restatement == reference
    python tools/make_golden_spatial_head.py --floor    # additionally measures the fp32 floor on the benchmark-sized clip (slow, ~10 GB)

The reference classes are imported at run time; what is stored is data.  ``prepare_multi_task`` needs the SigLIP text tower,
so what it would install is installed by hand: label tables as seeded unit vectors, the scale / bias pair, and ``w_v`` /
``v_proj`` / ``head_layernorm`` / ``head_mlp`` copied from a seeded encoder's pooling head exactly as modeling:1764-1779 does.

F16 cases (small config: image_size 48 -> 3 x 3 patches, hidden_size 128, intermediate_size 64, 4 frames):
  a  two clips with different mask widths: mask_size (96, 120) -> 48 x 60 and (64, 40) -> 48 x 30; 12 classes
  b  a normal clip and a clip whose mask is all background (loss 0, no gradient, still counted in the mean)
  c  130 classes (> 100): positives + random.sample negatives under random.seed(7), rows re-normalised
  d  TimesformerVideoClassificationHead: 3 clips, 10 classes
Per case: inputs (last_hidden_state as its seed + a checksum), the reference's loss, d last_hidden_state (d pooler_output for d), d logit_scale, d logit_bias and the gradients
of the ten projection tensors.  The projection parameters are regenerated from the seed (their SHA-256 is recorded).
``floor_*``: the fp32 evaluation of the reference's operator sequence (normalize -> einsum -> interpolate -> cross_entropy) against
the fp64 restatement on the same dense embeddings, max-abs error over the tensor's max-abs — the yardstick of the kernel's
gradient bound (tests/test_spatial_head.py).
"""
from __future__ import annotations

import copy
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "f16_vis_head.npz")

from oracle.make_golden import build_ref, import_reference, maxabs, small_cfg  # noqa: E402
from streamformer_amd.init_weights import make_state_dict, state_dict_sha256  # noqa: E402
from tests import spatial_head_oracle as S  # noqa: E402

SEED_WEIGHTS = 16
T_FRAMES = 4


unit_rows = S.unit_rows


def make_vis_head(ref_models, cfg, tables):
    sd = make_state_dict(cfg, seed=SEED_WEIGHTS)
    enc = build_ref(ref_models, cfg, sd)
    import models.modeling_timesformer_siglip as M
    head = M.TimesformerUniversalVideoInstanceSegmentationHead(enc.config, {k: {} for k in tables}, enc.head)
    # what prepare_multi_task (modeling:1739-1784) installs, without the text tower
    head.logit_scale = copy.deepcopy(torch.nn.Parameter(torch.log(torch.tensor(10.0))))
    head.logit_bias = copy.deepcopy(torch.nn.Parameter(torch.tensor(-2.0)))
    head.dataset_label_embeddings = dict(tables)
    D = cfg.hidden_size
    head.w_v = torch.nn.Linear(D, D, bias=True)
    head.w_v.weight.data = copy.deepcopy(enc.head.attention.in_proj_weight.data[2 * D:, :])
    head.w_v.bias.data = copy.deepcopy(enc.head.attention.in_proj_bias.data[2 * D:])
    head.v_proj = copy.deepcopy(enc.head.attention.out_proj)
    head.head_layernorm = copy.deepcopy(enc.head.layernorm)
    head.head_mlp = copy.deepcopy(enc.head.mlp)
    head.w_v.requires_grad = False            # as the reference: attributes on modules, freezing nothing
    head.v_proj.requires_grad = False
    head.head_layernorm.requires_grad = False
    head.head_mlp.requires_grad = False
    return head.train(), sd


def proj_params(head, dtype=torch.float32):
    named = dict(head.named_parameters())
    return {n: named[n].detach().clone().to(dtype).requires_grad_(True) for n in S.PROJ_NAMES}


def mask_floor(dense, tables, targets, ls, lb):
    """fp32 operator sequence vs fp64 restatement: relative max-abs error of d loss / d dense and of d loss / d (scale, bias)."""
    out = []
    for dt in (torch.float32, torch.float64):
        x = dense.detach().to(dt).requires_grad_(True)
        s, b = ls.detach().to(dt).requires_grad_(True), lb.detach().to(dt).requires_grad_(True)
        loss = S.mask_loss(x, [t.to(dt) for t in tables], targets, s, b)
        loss.backward()
        out.append((loss.detach(), x.grad, torch.stack([s.grad, b.grad])))
    (l32, g32, s32), (l64, g64, s64) = out
    return (float((l32.double() - l64).abs()), float((g32.double() - g64).abs().max() / g64.abs().max()),
            float((s32.double() - s64).abs().max() / s64.abs().max()))


def run_vis_case(tag, ref_models, cfg, tables, datasets, masks, sizes, lhs_seed, out, seed=None):
    head, sd = make_vis_head(ref_models, cfg, tables)
    B = len(datasets)
    lhs = S.seeded_randn(lhs_seed, B, T_FRAMES, cfg.num_patches, cfg.hidden_size).requires_grad_(True)
    if seed is not None:
        random.seed(seed)
    loss, _ = head(types.SimpleNamespace(last_hidden_state=lhs), {"dataset": datasets, "mask_target": masks, "mask_size": sizes})
    loss.backward()
    named = dict(head.named_parameters())
    # restatement, same draw
    p = proj_params(head)
    lhs2 = lhs.detach().clone().requires_grad_(True)
    ls, lb = named["logit_scale"].detach().clone().requires_grad_(True), named["logit_bias"].detach().clone().requires_grad_(True)
    if seed is not None:
        random.seed(seed)
    loss2 = S.vis_head_loss(lhs2, p, cfg.layer_norm_eps, tables, datasets, masks, sizes, cfg.image_size, ls, lb)
    loss2.backward()
    assert maxabs(loss2, loss) <= 1e-6, (tag, float(loss), float(loss2))
    assert maxabs(lhs2.grad, lhs.grad) <= 1e-7, (tag, maxabs(lhs2.grad, lhs.grad))
    assert maxabs(ls.grad, named["logit_scale"].grad) <= 1e-6 and maxabs(lb.grad, named["logit_bias"].grad) <= 1e-6, tag
    for n in S.PROJ_NAMES:
        assert named[n].grad is not None and float(named[n].grad.abs().max()) > 0, (tag, n, "the reference trains this tensor")
        assert maxabs(p[n].grad, named[n].grad) <= 1e-6, (tag, n, maxabs(p[n].grad, named[n].grad))
    # the selected tables / remapped targets the loss kernel is fed (same draw), and the fp32 floor on them
    if seed is not None:
        random.seed(seed)
    sel = [S.select_classes(tables[d], masks[i]) for i, d in enumerate(datasets)]
    with torch.no_grad():
        dense = S.dense_projection(lhs.detach(), {n: named[n].detach() for n in S.PROJ_NAMES}, cfg.layer_norm_eps)
    fl = mask_floor(dense, [t for t, _ in sel], [m for _, m in sel], named["logit_scale"], named["logit_bias"])
    print(f"  {tag}: loss {float(loss):.6f}  restatement == reference;  fp32 floor: loss {fl[0]:.2e}  d dense {fl[1]:.2e}  d scalars {fl[2]:.2e}")
    out[f"{tag}_lhs_seed"] = np.array(lhs_seed)               # inputs are regenerated from the seed; the sum detects RNG drift
    out[f"{tag}_lhs_sum"] = np.array(float(lhs.detach().double().sum()))
    out[f"{tag}_datasets"] = np.array(datasets)
    out[f"{tag}_mask_sizes"] = np.array(sizes, dtype=np.int64)
    for i, m in enumerate(masks):
        out[f"{tag}_mask{i}"] = m.numpy().astype(np.uint8)
    for i, (t, m) in enumerate(sel):
        out[f"{tag}_sel_target{i}"] = m.numpy().astype(np.int8)      # the remapped targets of the recorded draw (-1 = ignore)
    out[f"{tag}_loss"] = loss.detach().numpy()
    out[f"{tag}_d_lhs"] = lhs.grad.numpy()
    out[f"{tag}_d_logit_scale"] = named["logit_scale"].grad.numpy()
    out[f"{tag}_d_logit_bias"] = named["logit_bias"].grad.numpy()
    for n in S.PROJ_NAMES:
        out[f"{tag}_d_{n}"] = named[n].grad.numpy()
    out[f"{tag}_floor"] = np.array(fl, dtype=np.float64)
    if seed is not None:
        out[f"{tag}_random_seed"] = np.array(seed)
    return head, sd


def rand_mask(seed, W, H, classes, T=T_FRAMES):
    return S.blocky_mask(seed, T, H, W, classes)


def main():
    ref_models = import_reference()
    cfg = small_cfg(intermediate_size=64, num_frames=T_FRAMES)
    H, D = cfg.image_size, cfg.hidden_size
    out = {}
    print("F16: spatial head / classification head against the reference")
    tables = {"vis12": unit_rows(12, D, 1601), "vis130": unit_rows(130, D, 1602)}
    for k, v in tables.items():
        out[f"table_{k}"] = v.numpy()
    # a
    sizes = [(96, 120), (64, 40)]
    widths = [S.mask_width(H, s) for s in sizes]
    assert widths == [60, 30]
    masks = [rand_mask(1610 + i, w, H, list(range(12))) for i, w in enumerate(widths)]
    head, sd = run_vis_case("a", ref_models, cfg, {"vis12": tables["vis12"]}, ["vis12", "vis12"], masks, sizes, 1611, out)
    out["vis_param_names"] = np.array([n for n, _ in head.named_parameters()])
    out["vis_param_requires_grad"] = np.array([p.requires_grad for _, p in head.named_parameters()])
    out["state_dict_sha256"] = np.array(state_dict_sha256(sd))
    out["weights_seed"] = np.array(SEED_WEIGHTS)
    out["config"] = np.array(repr({"image_size": 48, "patch_size": 16, "hidden_size": 128, "intermediate_size": 64, "num_frames": T_FRAMES,
                                   "num_hidden_layers": 2, "num_attention_heads": 2}))
    # b
    sizes = [(48, 48), (48, 72)]
    masks = [rand_mask(1620, 48, H, list(range(12))), torch.zeros(T_FRAMES, H, 72, dtype=torch.long)]
    run_vis_case("b", ref_models, cfg, {"vis12": tables["vis12"]}, ["vis12", "vis12"], masks, sizes, 1621, out)
    # c
    sizes = [(48, 64), (96, 96)]
    masks = [rand_mask(1630, 64, H, [0, 3, 17, 64, 101, 129]), rand_mask(1631, 48, H, [0, 5, 99, 100, 128])]
    run_vis_case("c", ref_models, cfg, {"vis130": tables["vis130"]}, ["vis130", "vis130"], masks, sizes, 1632, out, seed=7)
    # d: classification head
    import models.modeling_timesformer_siglip as M
    chead = M.TimesformerVideoClassificationHead(cfg, {})
    chead.logit_scale = torch.nn.Parameter(torch.log(torch.tensor(10.0)))
    chead.logit_bias = torch.nn.Parameter(torch.tensor(-2.0))
    chead.label_embeddings = unit_rows(10, D, 1640)
    pooler = S.seeded_randn(1641, 3, T_FRAMES, D).requires_grad_(True)
    labels = torch.tensor([4, 0, 9])
    loss, _ = chead(types.SimpleNamespace(pooler_output=pooler), {"label": labels})
    loss.backward()
    p2 = pooler.detach().clone().requires_grad_(True)
    ls, lb = chead.logit_scale.detach().clone().requires_grad_(True), chead.logit_bias.detach().clone().requires_grad_(True)
    loss2 = S.classification_loss(p2, chead.label_embeddings, labels, ls, lb)
    loss2.backward()
    assert maxabs(loss2, loss) <= 1e-6 and maxabs(p2.grad, pooler.grad) <= 1e-7
    assert maxabs(ls.grad, chead.logit_scale.grad) <= 1e-6 and maxabs(lb.grad, chead.logit_bias.grad) <= 1e-6
    print(f"  d: loss {float(loss):.6f}  restatement == reference")
    out.update({"d_pooler": pooler.detach().numpy(), "d_table": chead.label_embeddings.numpy(), "d_labels": labels.numpy(),
                "d_loss": loss.detach().numpy(), "d_d_pooler": pooler.grad.numpy(), "d_d_logit_scale": chead.logit_scale.grad.numpy(),
                "d_d_logit_bias": chead.logit_bias.grad.numpy()})
    # fp32 floor on the benchmark-sized clip of the GPU test (16 x 196 x 768, L = 100, 224 x 398)
    if "--floor" in sys.argv:
        x, table, target = S.bench_clip_inputs()
        fl = mask_floor(x[None], [table], [target], torch.log(torch.tensor(10.0)), torch.tensor(-2.0))
        print(f"  benchmark-sized clip: fp32 floor: loss {fl[0]:.2e}  d dense {fl[1]:.2e}  d scalars {fl[2]:.2e}")
        out["bench_floor"] = np.array(fl, dtype=np.float64)
    elif os.path.exists(OUT) and "bench_floor" in np.load(OUT):
        out["bench_floor"] = np.load(OUT)["bench_floor"]
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
