"""Time per call of the native video-LLM connector against the reference's operator sequence in torch, on the same GPU, in the same process.

    python tools/connector_bench.py            # writes profiles/connector.txt

Shapes of the VideoQA recipe: D = 768 -> D_llm = 3584, mlp2x_gelu, a 14 x 14 grid, bilinear stride 2, newline position "grid", random
weights, F in {1, 8, 16} frames, both compute modes.  The torch side is the reference's order — projector on every patch token, then
F.interpolate, then the newline column (pool LAST) — in fp32 next to the accurate mode and in bf16 weights / activations (no autocast) next
to the bf16 mode.  Streaming: one ``StreamingVideoTokens.push`` of one frame (tower + connector on the new frame + window layout) against
what the reference does per streamed frame, the tower's call plus the torch tail on the whole 16-frame window it returns.

Method: every timed window is a batch of calls between two HIP events (at least ~50 ms of work), native and torch windows alternate, the
median (min) over the windows is reported, every shape is warmed up first; outputs of both sides are compared before anything is timed.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import streamformer_amd as sa  # noqa: E402
from tools._timing import compare  # noqa: E402

D_IN, D_OUT, P, STRIDE = 768, 3584, 14, 2
CONFIG = dict(mm_projector_type="mlp2x_gelu", mm_hidden_size=D_IN, hidden_size=D_OUT, mm_spatial_pool_stride=STRIDE,
              mm_spatial_pool_mode="bilinear", mm_newline_position="grid", mm_patch_merge_type="spatial_unpad")


def torch_tail(W, x):
    """The reference's sequence on x [F, P * P, D]: mm_projector, get_2dPool (bilinear), add_token_per_grid."""
    y = F.linear(F.gelu(F.linear(x, W["mm_projector.0.weight"], W["mm_projector.0.bias"])), W["mm_projector.2.weight"], W["mm_projector.2.bias"])
    n, _, c = y.shape
    g = y.view(n, P, P, c).permute(0, 3, 1, 2).contiguous()
    g = F.interpolate(g, size=[-(-P // STRIDE)] * 2, mode="bilinear").permute(0, 2, 3, 1)
    g = torch.cat([g, W["image_newline"].expand(n, g.shape[1], 1, c)], dim=2)
    return g.reshape(-1, c)
WINDOWS = dict(warmup=5, windows=9, target_ms=50.0)


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lines = [f"video-LLM connector, D {D_IN} -> {D_OUT}, mlp2x_gelu, {P} x {P} grid, bilinear stride {STRIDE}, newline grid; {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median (min) over alternating windows of >= 50 ms between HIP events; torch = the reference's order (pool last), same GPU, same process"]
    g = torch.Generator().manual_seed(0)
    sd = {"mm_projector.0.weight": torch.randn(D_OUT, D_IN, generator=g) / D_IN ** 0.5, "mm_projector.0.bias": 0.1 * torch.randn(D_OUT, generator=g),
          "mm_projector.2.weight": torch.randn(D_OUT, D_OUT, generator=g) / D_OUT ** 0.5, "mm_projector.2.bias": 0.1 * torch.randn(D_OUT, generator=g),
          "image_newline": torch.randn(D_OUT, generator=g) / D_OUT ** 0.5}
    feats = {n: torch.randn(n, P * P, D_IN, generator=g).to(dev) for n in (1, 8, 16)}
    conns = {}
    with torch.no_grad():
        for mode, tdtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            m = sa.VideoTokenConnector(CONFIG, compute_dtype=mode)
            m.load_state_dict(sd)
            m.to(dev)
            conns[mode] = m
            W = {k: v.to(dev, tdtype) for k, v in sd.items()}
            W32 = {k: v.to(dev) for k, v in sd.items()}
            for n, x in feats.items():
                got, want = m(x), torch_tail(W32, x)
                assert got.shape == want.shape
                lines.append(f"[{mode}] F = {n:2d}: {got.shape[0]} rows, max-abs against torch fp32 {float((got - want).abs().max()):.3e} (max |ref| {float(want.abs().max()):.2f})")
                xt = x.to(tdtype)
                nat_ms, t_ms = compare(lambda: m(x), lambda: torch_tail(W, xt), **WINDOWS)
                lines.append(f"[{mode}] F = {n:2d}: native {nat_ms[0]:.3f} ({nat_ms[1]:.3f}) ms   torch {tdtype} {t_ms[0]:.3f} ({t_ms[1]:.3f}) ms   "
                             f"torch / native {t_ms[0] / nat_ms[0]:.2f}")
        # streaming: SigLIP-base tower (64-frame sliding cache), a returned window of 16 frames, both streams filled before anything is timed
        cfg = sa.siglip_base()
        enc = sa.TimesformerMultiTaskingModelSigLIP(cfg, compute_dtype="bf16")
        enc.load_state_dict(sa.make_state_dict(cfg, seed=0))
        enc.to(dev).eval()
        frame = torch.randn(1, 1, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
        W = {k: v.to(dev, torch.bfloat16) for k, v in sd.items()}

        def filled(tower):
            tower.clear_cache()
            for _ in range(15):
                tower(frame)

        tower_a = sa.TimesformerVisionTower(enc, streaming_mode=True, context_length=16, max_frames=64, cache_policy="slide", compute_dtype="bf16")
        tower_b = sa.TimesformerVisionTower(enc, streaming_mode=True, context_length=16, max_frames=64, cache_policy="slide", compute_dtype="bf16")
        stream = sa.StreamingVideoTokens(tower_a, conns["bf16"])
        stream.clear()
        for _ in range(15):
            stream.push(frame)
        filled(tower_b)

        def reference_push():
            window = tower_b(frame)              # (1, 16, N, D): the whole window, as the reference's tower returns it
            return torch_tail(W, window[0].to(torch.bfloat16))

        a = stream.push(frame)
        b = reference_push()
        assert a.shape == b.shape
        lines.append(f"[streaming] window of 16 frames: {a.shape[0]} rows, max-abs native push against tower + torch bf16 tail {float((a - b.float()).abs().max()):.3e}")
        nat_ms, t_ms = compare(lambda: stream.push(frame), reference_push, **WINDOWS)
        lines.append(f"[streaming] one pushed frame, bf16: StreamingVideoTokens.push {nat_ms[0]:.3f} ({nat_ms[1]:.3f}) ms   tower + torch tail on the 16-frame window "
                     f"{t_ms[0]:.3f} ({t_ms[1]:.3f}) ms   ratio {t_ms[0] / nat_ms[0]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "connector.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
