"""Time of the native multi-scale deformable attention against the reference's operator sequence in torch, on the same GPU, in the same process.

    python tools/msda_bench.py            # writes profiles/msda.txt
    python tools/msda_bench.py --smoke    # one tiny shape, nothing written

Shapes: the Mask2Former pixel decoder (N = 2, d_model 256, 8 heads of 32, levels 48x80 / 24x40 / 12x20, Lq = S = 5040, 4 points) and the
ViT-Adapter around the encoder at 224^2 input (dim 768, 12 heads of 64, 4 points): the injector (196 queries over 28^2 + 14^2 + 7^2) and the
extractor (1029 queries over 14^2), at B T = 8 and 128 frames.

Timed: the operator forward, forward + backward, and the module's no-grad forward (four projections + the fused kernel, both compute
modes).  The torch side is what the reference runs without its CUDA extension (ms_deform_attn_core_pytorch): split per level, one
grid_sample per level, the weighted sum over levels and points, with torch autograd for the backward; for the module, nn.Linear, softmax
and the location arithmetic in front of it, in fp32.

Reported next to the times: for the forward the achieved bytes / s against the algorithmic minimum (value read once + output written
once); for the backward the atomic bytes / s (4 corners x D x 4 bytes per sample, every sample taken as inside) against the ~1.3 TB/s at
which the chip adds floats.

Method: every timed window is a batch of calls between two HIP events (at least ~50 ms of work), native and torch windows alternate, the
median (min) over the windows is reported, everything is warmed up first; results are compared before anything is timed.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import streamformer_amd as sa  # noqa: E402
from tools._timing import compare  # noqa: E402

ATOMIC_RATE = 1.3e12

SHAPES = [("pixel decoder", 2, 256, 8, [(48, 80), (24, 40), (12, 20)], 5040)]
for _frames in (8, 128):
    SHAPES.append((f"adapter injector, {_frames} frames", _frames, 768, 12, [(28, 28), (14, 14), (7, 7)], 196))
    SHAPES.append((f"adapter extractor, {_frames} frames", _frames, 768, 12, [(14, 14)], 1029))
SMOKE = [("smoke", 2, 64, 2, [(6, 5), (3, 3)], 11)]
P = 4


def torch_core(value, shapes, loc, w):
    N, S, M, D = value.shape
    Lq, L = loc.shape[1], loc.shape[3]
    grids = 2 * loc - 1
    sampled = []
    for l, v in enumerate(value.split([H * W for H, W in shapes], dim=1)):
        H, W = shapes[l]
        image = v.flatten(2).transpose(1, 2).reshape(N * M, D, H, W)
        sampled.append(F.grid_sample(image, grids[:, :, :, l].transpose(1, 2).flatten(0, 1), mode="bilinear", padding_mode="zeros", align_corners=False))
    weights = w.transpose(1, 2).reshape(N * M, 1, Lq, L * P)
    return (torch.stack(sampled, dim=-2).flatten(-2) * weights).sum(-1).view(N, M * D, Lq).transpose(1, 2).contiguous()


def torch_module(m, query, ref, flat, shapes):
    N, Lq, d = query.shape
    M, L = m.n_heads, m.n_levels
    value = m.value_proj(flat).view(N, -1, M, d // M)
    offsets = m.sampling_offsets(query).view(N, Lq, M, L, P, 2)
    w = F.softmax(m.attention_weights(query).view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    norm = torch.tensor([[W, H] for H, W in shapes], dtype=query.dtype, device=query.device)
    loc = ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
    return m.output_proj(torch_core(value, shapes, loc, w))


def row(label, nat_ms, t_ms, extra=""):
    return (f"  {label}: native {nat_ms[0]:.3f} ({nat_ms[1]:.3f}) ms   torch {t_ms[0]:.3f} ({t_ms[1]:.3f}) ms   torch / native "
            f"{t_ms[0] / nat_ms[0]:.2f}{extra}")


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    smoke = "--smoke" in sys.argv
    dev = torch.device("cuda:0")
    kw = dict(warmup=1, windows=2, target_ms=2.0, probe=2) if smoke else dict(warmup=3, windows=7, target_ms=50.0, probe=2)
    lines = [f"multi-scale deformable attention, {P} points; {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median (min) over alternating windows between HIP events; torch = the reference's sequence without its "
             "CUDA extension (per-level grid_sample + weighted sum, autograd backward), fp32, same GPU, same process"]
    g = torch.Generator().manual_seed(0)
    for label, N, d, M, shapes, Lq in (SMOKE if smoke else SHAPES):
        D, L, S = d // M, len(shapes), sum(H * W for H, W in shapes)
        lines.append(f"{label}: N {N}, d_model {d}, {M} heads of {D}, levels {shapes} (S = {S}), Lq {Lq}")
        value = torch.randn(N, S, M, D, generator=g).to(dev)
        loc = (torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.1 - 0.05).to(dev)
        w = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).to(dev)
        grad_out = torch.randn(N, Lq, M * D, generator=g).to(dev)
        with torch.no_grad():
            got, want = sa.ms_deform_attn(value, shapes, None, loc, w), torch_core(value, shapes, loc, w)
            lines.append(f"  forward max-abs against torch: {float((got - want).abs().max()):.3e} (max |ref| {float(want.abs().max()):.2f})")
            nat_ms, t_ms = compare(lambda: sa.ms_deform_attn(value, shapes, None, loc, w), lambda: torch_core(value, shapes, loc, w), **kw)
        minimum = 4.0 * (value.numel() + got.numel())
        lines.append(row("forward", nat_ms, t_ms, f"   {minimum / nat_ms[0] / 1e6:.1f} GB/s of the algorithmic minimum ({minimum / 1e6:.1f} MB)"))
        vg, lg, wg = (t.clone().requires_grad_(True) for t in (value, loc, w))

        def native_step():
            sa.ms_deform_attn(vg, shapes, None, lg, wg).backward(grad_out)
            vg.grad = lg.grad = wg.grad = None

        def torch_step():
            torch_core(vg, shapes, lg, wg).backward(grad_out)
            vg.grad = lg.grad = wg.grad = None

        nat_fb, t_fb = compare(native_step, torch_step, **kw)
        atomic = 4.0 * 4 * D * N * Lq * M * L * P
        bwd_ms = max(nat_fb[0] - nat_ms[0], 1e-6)
        lines.append(row("forward + backward", nat_fb, t_fb, f"   backward alone ~{bwd_ms:.3f} ms: {atomic / bwd_ms / 1e9:.3f} TB/s of atomic adds "
                                                                  f"({atomic / 1e6:.1f} MB) against ~{ATOMIC_RATE / 1e12:.1f} TB/s"))
        if d % 64 == 0:
            query, flat = torch.randn(N, Lq, d, generator=g).to(dev), torch.randn(N, S, d, generator=g).to(dev)
            ref = torch.rand(N, Lq, L, 2, generator=g).to(dev)
            for mode in ("fp32", "bf16"):
                m = sa.MSDeformAttn(d, L, M, P, compute_dtype=mode)
                with torch.no_grad():
                    m.sampling_offsets.weight.normal_(0, d ** -0.5, generator=g)
                    m.attention_weights.weight.normal_(0, d ** -0.5, generator=g)
                m = m.to(dev).eval()
                with torch.no_grad():
                    a, b = m(query, ref, flat, shapes, None), torch_module(m, query, ref, flat, shapes)
                    lines.append(f"  [{mode}] module max-abs against torch fp32: {float((a - b).abs().max()):.3e} (max |ref| {float(b.abs().max()):.2f})")
                    n_ms, tm_ms = compare(lambda: m(query, ref, flat, shapes, None), lambda: torch_module(m, query, ref, flat, shapes), **kw)
                lines.append(row(f"[{mode}] module forward, no grad", n_ms, tm_ms))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not smoke:
        with open(os.path.join(ROOT, "profiles", "msda.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
