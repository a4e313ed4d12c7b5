"""The tail models and the encoder on seeded weights and inputs, written to a file: the bit-identity check of a host-side change.

    python tools/tail_dump.py --case pixdec_fpn_enc2 --out a.pt [--root OTHER_TREE]
    python tools/tail_dump.py --case maskdec --out a.pt          # a model's name: every case of that model, one after the other
    python tools/tail_dump.py --case encoder --out a.pt          # enc_forward, enc_stream, enc_ops: the encoder's host code (below)
    python tools/tail_dump.py --case maskattn --out a.pt         # masked attention's entry points alone: forward, planes, stats, backward
    python tools/tail_dump.py --compare a.pt b.pt

A case builds one model (the smallest widths the GEMM k-step allows, a handful of rows), fills its parameters from a seeded generator,
runs it in both compute modes and saves every output tensor plus every ``*_workspace_bytes`` answer the module asked for on the way.
--root imports the package from another tree (a build of the parent commit).  --compare names every entry of two files that differs
(torch.equal for tensors) and exits non-zero if one does, or if the two files hold different entries."""
import argparse
import os
import sys

import numpy as np
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


# ---------------------------------------------------------------------------------------------------- the encoder
def small_encoder(sa, mode, dev):
    """The small golden configuration (tests/helpers.small_cfg) on seeded weights."""
    from streamformer_amd.init_weights import make_state_dict
    cfg = sa.StreamformerConfig(image_size=48, patch_size=16, num_frames=16, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                intermediate_size=256, enable_causal_temporal=True)
    m = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype=mode)
    m.load_state_dict(make_state_dict(cfg, seed=4))
    return m.to(dev).eval()


def run_enc_forward(sa, mode, g, dev):
    """sf_forward at B = 1 and 2 (with hidden states at B = 1), and sf_embed + sf_layers + sf_post_head staged."""
    m = small_encoder(sa, mode, dev)
    res = {}
    for B in (1, 2):
        x = torch.randn(B, 4, 3, 48, 48, generator=g).to(dev)
        o = m(x, output_hidden_states=B == 1)
        res[f"b{B}"] = {"last_hidden_state": o.last_hidden_state, "pooler_output": o.pooler_output, "hidden_states": o.hidden_states}
    h = m.embeddings(x)
    e = m.encoder(h, num_frames=4, output_attentions=True)
    y = m.post_layernorm(e.last_hidden_state)
    tok = y.reshape(B, 9, 4, 128).permute(0, 2, 1, 3).reshape(B * 4, 9, 128)      # patch-major tokens -> one row group per frame
    res["staged"] = {"embeddings": h, "encoder": e.last_hidden_state, "attentions": e.attentions, "post_layernorm": y, "head": m.head(tok)}
    return res


def run_enc_stream(sa, mode, g, dev):
    """Graphs on (the default): 6 single frames into a 4-frame sliding window; 3 streams staggered by one frame; one stream parked."""
    m = small_encoder(sa, mode, dev)
    pair = lambda o: {"last_hidden_state": o.last_hidden_state.clone(), "pooler_output": o.pooler_output.clone()}      # noqa: E731
    x = torch.randn(3, 7, 3, 48, 48, generator=g).to(dev)
    res = {}
    cache = m.new_cache(1, 4, policy="slide")
    for t in range(6):
        res[f"slide.{t}"] = pair(m(x[:1, t:t + 1], past_key_values=cache))
    cache = m.new_cache(3, 16)
    for t in range(6):      # stream i joins at call i
        ids = [i for i in range(3) if t >= i]
        xs = torch.stack([x[i, t - i] for i in ids])[:, None]
        res[f"ragged.{t}"] = pair(m(xs, past_key_values=cache, stream_ids=ids))
    snap = cache.snapshot(1)
    res["park.blob"] = snap.blob
    other = m.new_cache(2, 16)
    other.restore(snap, stream=1)
    res["park.resumed"] = pair(m(x[1:2, 5:6], past_key_values=other, stream_ids=[1]))
    res["park.prefill"] = pair(m(x[2:3, :3], past_key_values=other, stream_ids=[0]))      # several frames of one stream: the eager slab call
    return res


def gemm_call(nat, dev, g, family, M, N, K, split, resid):
    """One sf_op_gemm call on seeded planes (fp32 epilogue, or residual + bf16 copy); a refusal is recorded as its message."""
    import ctypes as C
    planes = lambda *shape: torch.randint(0x3c00, 0x4000, shape, generator=g, dtype=torch.int32).to(torch.int16).to(dev)      # noqa: E731
    a, w, bias, out = planes(M, K), planes(N, K), torch.randn(N, generator=g).to(dev), torch.zeros(M, N, device=dev)
    lo = [planes(M, K) >> 8, planes(N, K) >> 8] if split else []
    d = nat.SfGemmDesc()
    d.split, d.a_hi, d.w_hi, d.bias = int(split), a.data_ptr(), w.data_ptr(), bias.data_ptr()
    if split:
        d.a_lo, d.w_lo = lo[0].data_ptr(), lo[1].data_ptr()
    d.M, d.N, d.K, d.ldc, d.alpha, d.out_f32 = M, N, K, N, 0.75, out.data_ptr()
    d.epi = 3 if resid else 0      # SF_EPI_RESID_F32 / SF_EPI_F32
    if resid:
        out.copy_(torch.randn(M, N, generator=g))
        d.resid = out.data_ptr()
    taken = C.c_int(-1)
    rc = nat.lib.sf_op_gemm(C.byref(d), family, C.byref(taken), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if rc:
        return {"refused": torch.tensor(list(nat.lib.sf_last_error()), dtype=torch.uint8)}
    return {"out": out, "family": torch.tensor(taken.value)}


def run_enc_ops(sa, mode, g, dev):
    nat, heads = sa._native, sa.heads
    cm = nat.compute_mode(mode)
    stream = nat.current_stream_handle(dev)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
    res = {}
    M, N, K = 33, 64, 64
    x, w, b, r = rnd(M, K), rnd(N, K) / 8, rnd(N), rnd(M, N)
    nb = nat.lib.sf_op_linear_workspace_bytes(M, N, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    for name, resid, gelu in (("plain", None, 0), ("gelu", None, 1), ("resid", r, 0)):
        y = torch.empty(M, N, device=dev)
        nat.check(nat.lib.sf_op_linear(x.data_ptr(), w.data_ptr(), b.data_ptr(), nat.ptr(resid), 0.37 if resid is not None else 1.0, gelu, y.data_ptr(), M,
                                       N, K, cm, ws.data_ptr(), nb, stream))
        res[f"linear.{name}"] = y
    # one call per family (1 skinny .. 5 128^2) and the dispatcher's own choice (0) at the same shape
    for fam, shape in ((1, (33, 100, 64)), (2, (3136, 768, 128)), (3, (6272, 768, 128)), (4, (2048, 1024, 128)), (5, (600, 1000, 128))):
        for family in (fam, 0):
            for resid in (False, True):
                res[f"gemm.{fam}.{family}.{int(resid)}"] = gemm_call(nat, dev, g, family, *shape, split=mode == "fp32", resid=resid)
    for name, groups, L, temporal, causal, ntok, hd in (("spatial", 3, 17, 0, 0, 0, 64), ("temporal", 6, 5, 1, 1, 3, 64), ("spatial_hd32", 3, 17, 0, 0, 0, 32)):
        D = 2 * hd
        qkv, ctx = rnd(groups * L, 3 * D), torch.empty(groups * L, D, device=dev)
        nb = nat.lib.sf_op_attention_workspace_bytes(groups, L, 2, hd)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        nat.check(nat.lib.sf_op_attention(qkv.data_ptr(), ctx.data_ptr(), groups, L, 2, hd, causal, temporal, ntok, cm, ws.data_ptr(), nb, stream))
        res[f"attention.{name}"] = ctx
    B, T, D = 2, 3, 64
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)      # noqa: E731
    pooler = unit(rnd(B, T, D))
    res["loss.retrieval"] = heads.RetrievalHead().loss(pooler, unit(rnd(B, D)))
    res["loss.localization"] = heads.LocalizationHead(unit(rnd(5, D))).loss(pooler, torch.randint(0, 5, (B, T), generator=g))
    return res


# ---------------------------------------------------------------------------------------------------- masked attention, the operator alone
MASKATTN_SHAPES = ((8, 1, 1), (72, 17, 17), (32, 16, 31), (32, 100, 63), (128, 33, 130))      # (head width, Q, HW): one lane, a ragged last
# query tile, a ragged last key tile, a mask word boundary, more key tiles than waves, the widest head


def maskattn_mask(g, lead, Q, HW):
    """bool [*lead, Q, HW], True = hidden, and its packed words.  About half the bits; in the first [Q, HW] plane the last query is fully
    hidden and the last 16-key tile is hidden from the whole last 16-query tile (the skip path).  The properties are asserted."""
    m = torch.rand(*lead, Q, HW, generator=g) < 0.5
    first, q0, k0 = m.reshape(-1, Q, HW)[0], (Q - 1) // 16 * 16, (HW - 1) // 16 * 16
    first[Q - 1] = True
    first[q0:, k0:] = True
    assert bool(first[Q - 1].all()) and bool(first[q0:, k0:].all()) and first.data_ptr() == m.data_ptr()
    if m.numel() >= 512:
        assert 0.4 < float(m.float().mean()) < 0.75, float(m.float().mean())
    padded = torch.cat([m, torch.ones(*lead, Q, (-HW) % 32, dtype=torch.bool)], -1).numpy()      # the padding bits are set
    return m, torch.from_numpy(np.packbits(padded, axis=-1, bitorder="little").view(np.int32))      # uint32 bit patterns


def run_maskattn(sa, mode, g, dev):
    """sf_op_maskdec_attention (with and without k_pos, fp32 ctx and hi / lo planes), sf_op_maskattn_forward and sf_op_maskattn_backward."""
    nat = sa._native
    lib, stream, F, heads = nat.lib, nat.current_stream_handle(dev), 2, 2
    res = {}
    for hd, Q, HW in MASKATTN_SHAPES:
        D = heads * hd
        rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
        q, k, v, kpos, d_ctx = rnd(F * Q, D), rnd(F * HW, D), rnd(F * HW, D), rnd(HW, D), rnd(F * Q, D)
        for kind, lead in (("null", None), ("shared", (F,)), ("per_head", (F, heads))):
            words = None
            if lead is not None:
                words = maskattn_mask(g, lead, Q, HW)[1].to(dev)
            tag, mp, per_head = f"hd{hd}.q{Q}.hw{HW}.{kind}", nat.ptr(words), int(kind == "per_head")
            if kind != "per_head":      # the decoder's entry point takes one mask for all heads
                for name, pos in (("plain", None), ("kpos", kpos)):
                    ctx, hi, lo = torch.zeros(F * Q, D, device=dev), torch.zeros(F * Q, D, dtype=torch.int16, device=dev), torch.zeros(F * Q, D, dtype=torch.int16, device=dev)
                    nat.check(lib.sf_op_maskdec_attention(q.data_ptr(), D, k.data_ptr(), v.data_ptr(), D, nat.ptr(pos), D if pos is not None else 0, mp,
                                                          ctx.data_ptr(), hi.data_ptr(), lo.data_ptr(), F, Q, HW, heads, hd, 0, stream))
                    res[f"{tag}.maskdec.{name}"] = {"ctx": ctx, "hi": hi, "lo": lo}
            ctx, stats = torch.zeros(F * Q, D, device=dev), torch.zeros(F, heads, Q, device=dev)
            nat.check(lib.sf_op_maskattn_forward(q.data_ptr(), D, k.data_ptr(), v.data_ptr(), D, mp, per_head, ctx.data_ptr(), stats.data_ptr(), F, Q, HW,
                                                 heads, hd, 0, stream))
            dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
            nat.check(lib.sf_op_maskattn_backward(q.data_ptr(), D, k.data_ptr(), v.data_ptr(), D, mp, per_head, ctx.data_ptr(), stats.data_ptr(),
                                                  d_ctx.data_ptr(), dq.data_ptr(), D, dk.data_ptr(), dv.data_ptr(), D, F, Q, HW, heads, hd, 0, stream))
            res[f"{tag}.train"] = {"ctx": ctx, "stats": stats, "dq": dq, "dk": dk, "dv": dv}
    return res


CASES = {
    "maskattn": (run_maskattn, {}),
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
    "enc_forward": (run_enc_forward, {}),
    "enc_stream": (run_enc_stream, {}),
    "enc_ops": (run_enc_ops, {}),
}
MODELS = ("text", "connector", "oad", "pixdec", "maskdec", "enc")
FAMILIES = {"encoder": "enc"}      # --case encoder: every enc_* case
SIZERS = ("sf_text_workspace_bytes", "sf_connector_workspace_bytes", "sf_oad_workspace_bytes", "sf_pixdec_workspace_bytes",
          "sf_maskdec_workspace_bytes", "sf_workspace_bytes", "sf_stream_workspace_bytes", "sf_cache_stream_blob_bytes")
VALUE_SIZERS = ("sf_op_linear_workspace_bytes", "sf_op_attention_workspace_bytes", "sf_loss_workspace_bytes")      # the answer is the return value


def record_sizes(nat, log):
    """Every *_workspace_bytes call of the modules also appends its answer to ``log``."""
    for name in SIZERS:
        def wrapped(*args, _fn=getattr(nat.lib, name), _name=name):
            rc = _fn(*args)
            log.append((_name, int(args[-1]._obj.value)))
            return rc
        setattr(nat.lib, name, wrapped)
    for name in VALUE_SIZERS:
        def valued(*args, _fn=getattr(nat.lib, name), _name=name):
            n = _fn(*args)
            log.append((_name, int(n)))
            return n
        setattr(nat.lib, name, valued)


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
    wanted = [FAMILIES.get(n, n) for n in args.case]
    names = [c for n in wanted for c in CASES if c == n or (n in MODELS and c.startswith(n))]
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
