"""Training the Mask2Former masked-attention decoder on the MI355X: the two mask-logit entries alone, and forward + backward of the whole
decoder in training mode, against torch on the same GPU.

    python tools/mask_decoder_train_bench.py            # -> profiles/mask_decoder_train.txt
    python tools/mask_decoder_train_bench.py --smoke    # one tiny shape, a few iterations, no file

(a) entries  : sf_op_masklogits_forward + sf_op_masklogits_backward (both gradients, the workspace allocated outside the timed region)
               against ``torch.einsum("fqc,fcp->fqp")`` forward + autograd backward; F 16, Q 100, Dm 256, the 56 x 56 stride-4 grid of the
               224^2 config.  torch runs these products through its BLAS, whose fp32 path may use reduced-precision matrix
               instructions; the entries use exact fp32 products.
(b) decoder  : CLMultiScaleMaskedTransformerDecoder(trainable=True).train(): forward, a scalar pairing with every output (final and
               aux), backward; against the reference's operator sequence in torch with the same weights (tools/mask_decoder_bench.py's
               composition, keeping every head's prediction as the reference's _set_aux_loss does), and against that sequence after
               ``use_native_attention``.  F = 2 and 16; ``torch.cuda.max_memory_allocated`` of one step, measured from a reset peak.
Timing: warm-up steps, then HIP events around each step, medians (tools/_timing.py).  A cell where the native path loses is reported
as it is.
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import streamformer_amd as sa      # noqa: E402
import streamformer_amd._native as nat      # noqa: E402
from tools._timing import timed  # noqa: E402
from tools.pixel_decoder_bench import sine_table  # noqa: E402

KEYS = ("pred_logits", "pred_masks", "pred_queries", "pred_embeds")


def composed_train_forward(m, x, mask_features):
    """The reference's training forward in torch, [Q, B, C] order, with every head's prediction kept."""
    C, heads = m.hidden_dim, m.num_heads
    src, pos, sizes = [], [], []
    for i in range(3):
        sizes.append(x[i].shape[-2:])
        pos.append(sine_table(x[i], C).flatten(2).expand(x[i].shape[0], -1, -1).permute(2, 0, 1))
        p = m.input_proj[i]
        y = F.conv2d(x[i], p.weight, p.bias) if isinstance(p, sa.pixel_decoder.ConvNorm) else x[i]
        src.append((y.flatten(2) + m.level_embed.weight[i][None, :, None]).permute(2, 0, 1))
    bs = src[0].shape[1]
    qe = m.query_embed.weight.unsqueeze(1).repeat(1, bs, 1)
    out = m.query_feat.weight.unsqueeze(1).repeat(1, bs, 1)

    def mlp(mod, v):
        n = len(mod.layers)
        for j, layer in enumerate(mod.layers):
            v = F.relu(layer(v)) if j < n - 1 else layer(v)
        return v

    def heads_of(out, size):
        dn = m.decoder_norm(out).transpose(0, 1)
        pm = torch.einsum("bqc,bchw->bqhw", mlp(m.mask_embed, dn), mask_features)
        am = F.interpolate(pm, size=size, mode="bilinear", align_corners=False)
        am = (am.sigmoid().flatten(2).unsqueeze(1).repeat(1, heads, 1, 1).flatten(0, 1) < 0.5).bool().detach()
        emb = dn if isinstance(m.reid_embed, torch.nn.Identity) else mlp(m.reid_embed, dn)
        return dict(pred_logits=m.class_embed(dn), pred_masks=pm, pred_queries=dn, pred_embeds=emb), am

    preds = []
    pred, am = heads_of(out, sizes[0])
    preds.append(pred)
    for i in range(m.num_layers):
        l = i % 3
        am[torch.where(am.sum(-1) == am.shape[-1])] = False
        ca, sl, ff = m.transformer_cross_attention_layers[i], m.transformer_self_attention_layers[i], m.transformer_ffn_layers[i]
        out = ca.norm(out + ca.multihead_attn(query=out + qe, key=src[l] + pos[l], value=src[l], attn_mask=am)[0])
        out = sl.norm(out + sl.self_attn(out + qe, out + qe, value=out)[0])
        out = ff.norm(out + ff.linear2(F.relu(ff.linear1(out))))
        pred, am = heads_of(out, sizes[(i + 1) % 3])
        preds.append(pred)
    return preds


def step(forward, module, xs, mf):
    """Forward, a pairing with every output, backward to the parameters and the inputs."""
    module.zero_grad(set_to_none=True)
    for t in xs + [mf]:
        t.grad = None
    preds = forward()
    sum(p[k].square().mean() for p in preds for k in KEYS).backward()


def measure(fn, warmup, iters):
    ms = timed(fn, warmup=warmup, iters=iters)[0]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return ms, torch.cuda.max_memory_allocated() / 2 ** 20


def entries(lines, Fr, Q, Dm, H, W, warmup, iters, dev):
    P = H * W
    me, feat, dl = (torch.randn(*s, device=dev) for s in ((Fr, Q, Dm), (Fr, Dm, P), (Fr, Q, P)))
    out, d_me, d_feat = torch.empty(Fr, Q, P, device=dev), torch.empty_like(me), torch.empty_like(feat)
    ws = torch.empty(nat.lib.sf_op_masklogits_backward_workspace_bytes(Fr, Q, Dm, P), dtype=torch.uint8, device=dev)
    stream = nat.current_stream_handle(dev)

    def fwd():
        nat.check(nat.lib.sf_op_masklogits_forward(me.data_ptr(), feat.data_ptr(), out.data_ptr(), Fr, Q, Dm, P, stream))

    def bwd():
        nat.check(nat.lib.sf_op_masklogits_backward(dl.data_ptr(), me.data_ptr(), feat.data_ptr(), d_me.data_ptr(), d_feat.data_ptr(), 0, Fr, Q, Dm, P,
                                                    ws.data_ptr(), ws.numel(), stream))

    me_t, feat_t = me.clone().requires_grad_(), feat.clone().requires_grad_()
    state = {}

    def t_fwd():
        state["out"] = torch.einsum("fqc,fcp->fqp", me_t, feat_t)

    def t_bwd():
        me_t.grad = feat_t.grad = None
        state["out"].backward(dl, retain_graph=True)

    n_f, n_b = timed(fwd, warmup, iters)[0], timed(bwd, warmup, iters)[0]
    t_f = timed(t_fwd, warmup, iters)[0]
    t_b = timed(t_bwd, warmup, iters)[0]
    flop = 2.0 * Fr * Q * Dm * P
    worst = max(float((out - state["out"].detach()).abs().max()), float((d_me - me_t.grad).abs().max()), float((d_feat - feat_t.grad).abs().max()))
    lines.append(f"(a) entries F={Fr} Q={Q} Dm={Dm} P={H}x{W}: forward native {n_f:.3f} ({flop / n_f / 1e9:.1f} TFLOP/s), einsum {t_f:.3f}; backward native "
                 f"{n_b:.3f} ({2 * flop / n_b / 1e9:.1f} TFLOP/s), autograd {t_b:.3f}; workspace {ws.numel() / 2 ** 20:.1f} MiB; largest difference {worst:.1e}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--smoke", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[2, 16])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda:0")
    if args.smoke:
        cfg = dict(hidden=64, heads=8, ffn=128, layers=4, queries=20, mask_dim=64, classes=5, reid=2, grids=[(12, 20), (6, 10), (3, 5), (2, 3)])
        args.frames, args.iters, args.warmup = [2], 2, 1
    else:
        cfg = dict(hidden=256, heads=8, ffn=2048, layers=9, queries=100, mask_dim=256, classes=40, reid=3, grids=[(56, 56), (28, 28), (14, 14), (7, 7)])
    lines = [f"mask decoder training step, hidden {cfg['hidden']}, {cfg['heads']} heads, ffn {cfg['ffn']}, {cfg['layers']} layers, {cfg['queries']} queries, "
             f"mask_dim {cfg['mask_dim']}, {cfg['classes']} classes, {cfg['reid']} reid layers, grids {cfg['grids']}; fp32; median of {args.iters} after "
             f"{args.warmup} warm-up, HIP events; milliseconds, peak MiB of one step"]
    H, W = cfg["grids"][0]
    entries(lines, 2 if args.smoke else 16, cfg["queries"], cfg["mask_dim"], H, W, args.warmup, args.iters, dev)
    torch.manual_seed(0)
    m = sa.CLMultiScaleMaskedTransformerDecoder(cfg["hidden"], num_classes=cfg["classes"], hidden_dim=cfg["hidden"], num_queries=cfg["queries"],
                                                nheads=cfg["heads"], dim_feedforward=cfg["ffn"], dec_layers=cfg["layers"], pre_norm=False,
                                                mask_dim=cfg["mask_dim"], enforce_input_project=False, reid_hidden_dim=cfg["hidden"],
                                                num_reid_head_layers=cfg["reid"], trainable=True).to(dev).train()
    torch.nn.init.normal_(m.mask_embed.layers[2].bias, mean=0.5, std=0.1)      # masks that hide about half of the keys, not all or none
    m_attn = copy.deepcopy(m)
    swapped = sa.use_native_attention(m_attn)
    assert swapped == 2 * cfg["layers"], swapped
    for Fr in args.frames:
        mf = torch.randn(Fr, cfg["mask_dim"], H, W, device=dev).requires_grad_()
        xs = [torch.randn(Fr, cfg["hidden"], h, w, device=dev).requires_grad_() for h, w in cfg["grids"][:0:-1]]

        def native():
            out = m(xs, mf)
            return out["aux_outputs"] + [out]

        cells = []
        for what, fn, mod in (("native", native, m), ("torch", lambda: composed_train_forward(m, xs, mf), m),
                              ("torch + use_native_attention", lambda: composed_train_forward(m_attn, xs, mf), m_attn)):
            ms, peak = measure(lambda: step(fn, mod, xs, mf), args.warmup, args.iters)
            cells.append(f"{what} {ms:.2f} ms, peak {peak:.0f} MiB")
        lines.append(f"(b) decoder forward + backward F={Fr}: " + "; ".join(cells))
        print(lines[-1], flush=True)
        del mf, xs
        torch.cuda.empty_cache()
    if not args.smoke:
        path = os.path.join(ROOT, "profiles", "mask_decoder_train.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(path)


if __name__ == "__main__":
    main()
