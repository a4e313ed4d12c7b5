"""The tail models on seeded weights and inputs, written to a file: the bit-identity check of a host-side change to their handles.

    python tools/tail_dump.py --case pixdec_fpn_enc2 --out a.pt [--root OTHER_TREE]
    python tools/tail_dump.py --case maskdec --out a.pt          # a model's name: every case of that model, one after the other
    python tools/tail_dump.py --compare a.pt b.pt

A case builds one model (the smallest widths the GEMM k-step allows, a handful of rows), fills its parameters from a seeded generator,
runs it in both compute modes and saves every output tensor plus every ``*_workspace_bytes`` answer the module asked for on the way.
--root imports the package from another tree (a build of the parent commit).  --compare names every entry of two files that differs
(torch.equal for tensors) and exits non-zero if one does, or if the two files hold different entries."""
import argparse
import os
import sys

import torch

MODES = ("fp32", "bf16")
LEVELS = ("res2", "res3", "res4", "res5")
GRIDS = {"res2": (12, 20), "res3": (6, 10), "res4": (3, 5), "res5": (2, 3)}


def seed_parameters(module, g):
    """Every parameter from the generator: matrices ~ 1 / sqrt(fan_in), norm gains around 1, biases around 0."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / (p.numel() // p.shape[0]) ** 0.5)
            else:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))


def flatten(prefix, value, out):
    if torch.is_tensor(value):
        out[prefix] = value.detach().cpu()
    elif isinstance(value, dict):
        for k, v in value.items():
            flatten(f"{prefix}.{k}", v, out)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            flatten(f"{prefix}.{i}", v, out)
    elif value is not None:
        raise TypeError(f"{prefix}: {type(value)}")


# ---------------------------------------------------------------------------------------------------- the models
def run_text(sa, mode, g, dev):
    cfg = sa.SiglipTextConfig(vocab_size=100, hidden_size=64, intermediate_size=100, num_hidden_layers=2, num_attention_heads=4,
                              max_position_embeddings=16, projection_size=48)      # intermediate 100: the zero-padded MLP
    m = sa.SiglipTextModel(cfg, compute_dtype=mode)
    seed_parameters(m, g)
    m.to(dev)
    ids = torch.randint(0, cfg.vocab_size, (6, 10), generator=g).to(dev)
    mask = (torch.arange(10)[None] < torch.tensor([10, 3, 7, 1, 9, 5])[:, None]).long().to(dev)
    out = m(ids, attention_mask=mask)
    return {"last_hidden_state": out[0], "pooler_output": out[1], "groups": m.encode_groups(ids, 3), "groups_masked": m.encode_groups(ids, 2, mask)}


def run_connector(sa, mode, g, dev, projector):
    res = {}
    feats = torch.randn(3, 25, 64, generator=g).to(dev)      # a 5 x 5 grid: bilinear leaves 3 x 3 cells, the pools 2 x 2
    newline = {"no_token": ("flat", "one_token"), "one_token": ("spatial_unpad", "one_token"), "frame": ("spatial", "frame"),
               "grid": ("spatial", "grid")}
    for pool, stride in (("average", 2), ("max", 2), ("bilinear", 2), ("bilinear", 1)):
        for nl, (merge, position) in newline.items():
            m = sa.VideoTokenConnector(dict(mm_projector_type=projector, mm_hidden_size=64, hidden_size=128, mm_spatial_pool_stride=stride,
                                            mm_spatial_pool_mode=pool, mm_newline_position=position, mm_patch_merge_type=merge),
                                       compute_dtype=mode)
            seed_parameters(m, g)
            m.to(dev)
            res[f"{pool}{stride}.{nl}"] = m(feats)
    return res


def run_oad(sa, mode, g, dev, linear):
    cfg = sa.OADConfig(VISUAL_SIZE=64, NUM_CLASSES=5, LINEAR_ENABLED=linear, LINEAR_OUT_FEATURES=64, NUM_HEADS=4, DIM_FEEDFORWARD=128,
                       LONG_MEMORY_NUM_SAMPLES=8, WORK_MEMORY_NUM_SAMPLES=4, ENC_MODULE=[[4, 1, True], [6, 2, True], [-1, 1, False]],
                       DEC_MODULE=[-1, 2, True])
    det = sa.OnlineActionDetector(cfg, compute_dtype=mode)
    seed_parameters(det, g)
    det.to(dev)
    L, W = cfg.LONG_MEMORY_NUM_SAMPLES, cfg.WORK_MEMORY_NUM_SAMPLES
    state = det.new_state(2)
    mask = torch.zeros(L)
    mask[:2] = float("-inf")
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
    res = {"first": det.step(rnd(2, W, 64), rnd(2, L, 64), mask, state=state)}
    res["pushed"] = det.step(rnd(2, W, 64), rnd(2, 1, 64), mask, state=state)
    res["none"] = det.step(rnd(2, W, 64), None, None, state=state, probs=True)
    res["mixed"] = det.step(rnd(2, W, 64), [None, rnd(1, 64)], mask, state=state)
    res["one_stream"] = det.step(rnd(1, W, 64), rnd(1, 1, 64), None, state=state, stream_ids=[1])
    return res


def run_pixdec(sa, mode, g, dev, levels, transformer, enc_layers, stride):
    m = sa.MSDeformAttnPixelDecoder({k: sa.ShapeSpec(64, 4 << LEVELS.index(k)) for k in levels}, transformer_dropout=0.0, transformer_nheads=8,
                                    transformer_dim_feedforward=128, transformer_enc_layers=enc_layers, conv_dim=64, mask_dim=64, norm="GN",
                                    transformer_in_features=list(transformer), common_stride=stride, compute_dtype=mode, im2col_chunk_rows=100)
    seed_parameters(m, g)
    m = m.to(dev).eval()
    feats = {k: torch.randn(2, 64, *GRIDS[k], generator=g).to(dev) for k in levels}
    mask_features, first, multi_scale = m.forward_features(feats)
    return {"mask_features": mask_features, "first": first, "multi_scale": multi_scale}


def run_maskdec(sa, mode, g, dev, in_channels, reid, dec_layers):
    kw = dict(num_classes=5, hidden_dim=64, num_queries=20, nheads=8, dim_feedforward=128, dec_layers=dec_layers, pre_norm=False, mask_dim=64,
              enforce_input_project=False, compute_dtype=mode)
    if reid < 0:
        m = sa.MultiScaleMaskedTransformerDecoder(in_channels, **kw)
    else:
        m = sa.CLMultiScaleMaskedTransformerDecoder(in_channels, reid_hidden_dim=128, num_reid_head_layers=reid, **kw)
    seed_parameters(m, g)
    m = m.to(dev).eval()
    x = [torch.randn(2, in_channels, *GRIDS[k], generator=g).to(dev) for k in ("res5", "res4", "res3")]
    mask_features = torch.randn(2, 64, *GRIDS["res2"], generator=g).to(dev)
    return {"plain": m(x, mask_features), "aux": m(x, mask_features, return_aux=True, return_attn_masks=True)}


CASES = {
    "text": (run_text, {}),
    "connector_depth1": (run_connector, dict(projector="linear")),
    "connector_depth2": (run_connector, dict(projector="mlp2x_gelu")),
    "connector_depth3": (run_connector, dict(projector="mlp3x_gelu")),      # the ping-pong activation planes
    "oad_linear": (run_oad, dict(linear=True)),
    "oad_nolinear": (run_oad, dict(linear=False)),
    "pixdec_fpn_enc2": (run_pixdec, dict(levels=LEVELS, transformer=LEVELS[1:], enc_layers=2, stride=4)),
    "pixdec_fpn_enc0": (run_pixdec, dict(levels=LEVELS, transformer=LEVELS[1:], enc_layers=0, stride=4)),
    "pixdec_nofpn_enc2": (run_pixdec, dict(levels=LEVELS[1:], transformer=LEVELS[1:], enc_layers=2, stride=8)),
    "pixdec_nofpn_enc0": (run_pixdec, dict(levels=LEVELS[1:], transformer=LEVELS[1:], enc_layers=0, stride=8)),
    "pixdec_skip_level": (run_pixdec, dict(levels=LEVELS, transformer=("res3", "res5"), enc_layers=2, stride=4)),      # res4 is not used at all
    "pixdec_two_fpn": (run_pixdec, dict(levels=LEVELS, transformer=("res4", "res5"), enc_layers=2, stride=4)),
    "maskdec_proj_reid3": (run_maskdec, dict(in_channels=128, reid=3, dec_layers=4)),
    "maskdec_noproj_reid0": (run_maskdec, dict(in_channels=64, reid=0, dec_layers=4)),
    "maskdec_noproj_base": (run_maskdec, dict(in_channels=64, reid=-1, dec_layers=4)),
    "maskdec_proj_layers0": (run_maskdec, dict(in_channels=128, reid=3, dec_layers=0)),
    "maskdec_noproj_reid1": (run_maskdec, dict(in_channels=64, reid=1, dec_layers=1)),
}
MODELS = ("text", "connector", "oad", "pixdec", "maskdec")
SIZERS = ("sf_text_workspace_bytes", "sf_connector_workspace_bytes", "sf_oad_workspace_bytes", "sf_pixdec_workspace_bytes",
          "sf_maskdec_workspace_bytes")


def record_sizes(nat, log):
    """Every *_workspace_bytes call of the modules also appends its answer to ``log``."""
    for name in SIZERS:
        def wrapped(*args, _fn=getattr(nat.lib, name), _name=name):
            rc = _fn(*args)
            log.append((_name, int(args[-1]._obj.value)))
            return rc
        setattr(nat.lib, name, wrapped)


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    bad = [k for k in a if k not in b or (not torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] != b[k])]
    bad += [k for k in b if k not in a]
    for k in bad:
        print(f"  {k}: DIFFERS")
    print(f"{len(a)} entries, {len(bad)} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", help="case names, or a model's name for all of its cases: " + ", ".join(sorted(CASES)))
    ap.add_argument("--out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    names = [c for n in args.case for c in CASES if c == n or (n in MODELS and c.startswith(n))]
    if not names or not args.out:
        ap.error("--case needs known names and --out a file")
    sys.path.insert(0, os.path.abspath(args.root))
    import streamformer_amd as sa
    import streamformer_amd._native as nat

    dev = torch.device("cuda:0")
    sizes, out = [], {}
    record_sizes(nat, sizes)
    with torch.no_grad():
        for name in names:
            fn, kw = CASES[name]
            for mode in MODES:
                del sizes[:]
                flatten(f"{name}.{mode}", fn(sa, mode, torch.Generator().manual_seed(7), dev, **kw), out)
                torch.cuda.synchronize()
                out[f"{name}.{mode}.workspace_bytes"] = list(sizes)
                print(f"{name} [{mode}]: workspace_bytes {sorted(set(n for _, n in sizes))}", flush=True)
    torch.save(out, args.out)
    tensors = [v for v in out.values() if torch.is_tensor(v)]
    finite = all(bool(torch.isfinite(v.float()).all()) for v in tensors)
    print(f"wrote {args.out}: {len(tensors)} tensors, all finite: {finite}", flush=True)


if __name__ == "__main__":
    main()
