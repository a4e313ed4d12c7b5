"""Helper of the multi-scale deformable attention tests (not a test file): the operator and the ``MSDeformAttn`` module restated in torch
at a chosen precision.  Nothing here imports the package under test or the reference.

    core(value, shapes, loc, w)         the operator as an explicit four-corner gather: pixel = loc * size - 0.5, a sample counts iff
                                        -1 < h < H and -1 < w < W, every corner bounds-checked on its own (the CUDA kernel's rule, equal to
                                        grid_sample(bilinear, zeros, align_corners=False)).  Differentiable: torch autograd on it gives the
                                        analytic gradients (floor() has no gradient, the corner weights carry all of it).
    core_grid_sample(...)               the REFERENCE'S operator sequence (split per level, grid_sample, weighted sum): in fp32 it is the
                                        precision floor of the GPU tests, in fp64 it must agree with core().
    locations(...), module(...)         the front of MSDeformAttn.forward and the whole module; ``bf16_operands="x3"`` / ``True`` round the
                                        operands of every Linear as the library's two compute modes do (tests/oracle_ops.py).

Fixture F21 (tests/golden/f21_msda.npz, written by tools/make_golden_msda.py from the reference's own classes in fp64): per case the
inputs, the outputs and the autograd gradients; module weights are redrawn from the stored seed by make_weights().
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.oracle_ops import operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f21_msda.npz")

# operator cases of the fixture: N = 2 throughout
CORE_CASES = {
    "c0": dict(M=2, D=8, shapes=[(6, 5), (3, 3), (1, 2)], P=4, Lq=5, seed=2101),
    "c1": dict(M=3, D=32, shapes=[(3, 4)], P=1, Lq=3, seed=2102),
}
# module cases of the fixture; grads: parameter and input gradients are stored too
MODULE_CASES = {
    "tiny": dict(d_model=64, heads=2, shapes=[(3, 4), (2, 2)], P=2, Lq=3, ref_dim=2, mask=True, grads=True, seed=2111),
    "tiny4": dict(d_model=32, heads=2, shapes=[(2, 3), (1, 2)], P=2, Lq=3, ref_dim=4, mask=False, grads=True, seed=2122),
    "pix": dict(d_model=256, heads=8, shapes=[(2, 3), (2, 2), (1, 2)], P=4, Lq=4, ref_dim=2, mask=True, grads=False, seed=2113),
    "ada1": dict(d_model=768, heads=12, shapes=[(2, 3)], P=4, Lq=2, ref_dim=2, mask=False, grads=False, seed=2114),
    "ada3": dict(d_model=768, heads=12, shapes=[(2, 2), (1, 2), (1, 1)], P=4, Lq=2, ref_dim=4, mask=False, grads=False, seed=2115),
}
PARAMS = ("sampling_offsets", "attention_weights", "value_proj", "output_proj")
N_BATCH = 2
MIN_FRACTION = 1e-3      # distance of every gradient case's pixel coordinates from an integer (the gradient jumps there)


def level_starts(shapes):
    out, acc = [], 0
    for H, W in shapes:
        out.append(acc)
        acc += H * W
    return out


def pixels(shapes):
    return sum(H * W for H, W in shapes)


def pixel_coordinates(loc, shapes):
    """[N, Lq, M, L, P, 2] of (w_im, h_im) in fp64."""
    size = torch.tensor([[W, H] for H, W in shapes], dtype=torch.float64)
    return loc.double() * size[None, None, None, :, None, :] - 0.5


def away_from_integers(loc, shapes, margin=MIN_FRACTION):
    px = pixel_coordinates(loc, shapes)
    return bool(((px - px.round()).abs() >= margin).all())


def draw_locations(rs, N, Lq, M, shapes, P, lo=-0.2, hi=1.2):
    """fp32 locations uniform over [lo, hi] — inside, straddling every border, wholly outside — redrawn where a pixel coordinate comes
    within MIN_FRACTION of an integer; the result is asserted, in fp64, to satisfy that condition."""
    L = len(shapes)
    loc = torch.from_numpy(rs.uniform(lo, hi, (N, Lq, M, L, P, 2)).astype(np.float32))
    for _ in range(64):
        px = pixel_coordinates(loc, shapes)
        bad = (px - px.round()).abs() < 2 * MIN_FRACTION
        if not bad.any():
            break
        fresh = torch.from_numpy(rs.uniform(lo, hi, tuple(loc.shape)).astype(np.float32))
        loc = torch.where(bad, fresh, loc)
    assert away_from_integers(loc, shapes), "a sample sits on a pixel boundary: the location gradient is not defined there"
    return loc


def core(value, shapes, loc, w, padding_mask=None):
    """value [N, S, M, D], loc [N, Lq, M, L, P, 2], w [N, Lq, M, L, P] -> [N, Lq, M * D] in value's dtype."""
    N, S, M, D = value.shape
    Lq, P = loc.shape[1], loc.shape[4]
    if padding_mask is not None:
        value = value.masked_fill(padding_mask[:, :, None, None], 0.0)
    out = value.new_zeros(N, Lq, M, D)
    start = 0
    for l, (H, W) in enumerate(shapes):
        v = value[:, start:start + H * W].permute(0, 2, 1, 3)                    # [N, M, H W, D]
        x = loc[:, :, :, l, :, 0] * W - 0.5                                      # [N, Lq, M, P]
        y = loc[:, :, :, l, :, 1] * H - 0.5
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
        x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
        lx, ly = x - x0, y - y0
        for dy, dx, weight in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            yy, xx = y0 + dy, x0 + dx
            live = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (torch.nan_to_num(yy).clamp(0, H - 1) * W + torch.nan_to_num(xx).clamp(0, W - 1)).long()
            idx = idx.permute(0, 2, 1, 3).reshape(N, M, Lq * P, 1).expand(-1, -1, -1, D)
            taken = torch.gather(v, 2, idx).reshape(N, M, Lq, P, D).permute(0, 2, 1, 3, 4)      # [N, Lq, M, P, D]
            coef = torch.where(live, weight * w[:, :, :, l, :], torch.zeros_like(weight))
            out = out + (coef[..., None] * taken).sum(3)
        start += H * W
    return out.reshape(N, Lq, M * D)


def core_grid_sample(value, shapes, loc, w):
    """The reference's operator sequence in torch: per level, the level's pixels as an image per (sample, head), grid_sample at
    2 loc - 1, then the weighted sum over levels and points."""
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    grids = 2 * loc - 1
    sampled, start = [], 0
    for l, (H, W) in enumerate(shapes):
        image = value[:, start:start + H * W].flatten(2).transpose(1, 2).reshape(N * M, D, H, W)
        grid = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)                   # [N M, Lq, P, 2]
        sampled.append(F.grid_sample(image, grid, mode="bilinear", padding_mode="zeros", align_corners=False))      # [N M, D, Lq, P]
        start += H * W
    weights = w.transpose(1, 2).reshape(N * M, 1, Lq, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * weights).sum(-1).view(N, M * D, Lq)
    return out.transpose(1, 2).contiguous()


def core_with_grads(fn, value, shapes, loc, w, grad_out):
    """(out, grad_value, grad_loc, grad_w) of ``fn`` by torch autograd."""
    value, loc, w = (t.detach().clone().requires_grad_(True) for t in (value, loc, w))
    out = fn(value, shapes, loc, w)
    gv, gl, gw = torch.autograd.grad(out, (value, loc, w), grad_out)
    return out.detach(), gv, gl, gw


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
def weight_shapes(c):
    d, n = c["d_model"], c["heads"] * len(c["shapes"]) * c["P"]
    return {"sampling_offsets.weight": (2 * n, d), "sampling_offsets.bias": (2 * n,), "attention_weights.weight": (n, d), "attention_weights.bias": (n,),
            "value_proj.weight": (d, d), "value_proj.bias": (d,), "output_proj.weight": (d, d), "output_proj.bias": (d,)}


def make_weights(c, seed=None):
    """fp32 state dict under the reference's names: matrices N(0, 1 / fan_in), biases N(0, 0.1^2), the sampling-offset weight and bias
    scaled so that offsets spread over a few pixels; numpy.random.RandomState streams are frozen across NumPy versions."""
    rs = np.random.RandomState(c["seed"] if seed is None else seed)
    sd = {}
    for k, shape in weight_shapes(c).items():
        z = rs.standard_normal(shape)
        if k == "sampling_offsets.bias":
            v = 1.5 * z
        elif k.endswith("bias"):
            v = 0.1 * z
        else:
            v = z / np.sqrt(shape[1])
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def make_module_inputs(c, seed=None):
    """query, input_flatten [N, *, d_model], reference_points [N, Lq, L, ref_dim], padding mask or None, grad_out: values that bf16 and
    fp16 hold exactly are not needed here, but the fixture stores them as fp16, so they are rounded to it."""
    rs = np.random.RandomState((c["seed"] if seed is None else seed) + 7)
    d, Lq, shapes = c["d_model"], c["Lq"], c["shapes"]
    S, L = pixels(shapes), len(shapes)

    def half(a):
        return torch.from_numpy(a.astype(np.float16).astype(np.float32))

    query = half(rs.standard_normal((N_BATCH, Lq, d)))
    flat = half(rs.standard_normal((N_BATCH, S, d)))
    ref = rs.uniform(0.05, 0.95, (N_BATCH, Lq, L, 2))
    if c["ref_dim"] == 4:
        ref = np.concatenate([ref, rs.uniform(0.2, 0.9, (N_BATCH, Lq, L, 2))], -1)
    ref = half(ref)
    mask = None
    if c["mask"]:
        mask = torch.from_numpy(rs.uniform(size=(N_BATCH, S)) < 0.25)
        mask[1, level_starts(shapes)[-1]:] = True          # the last level of sample 1 is padding altogether
    grad_out = half(rs.standard_normal((N_BATCH, Lq, d)))
    return query, flat, ref, mask, grad_out


def locations(offsets, ref, shapes, P):
    """offsets [N, Lq, M, L, P, 2] (raw Linear output), ref [N, Lq, L, 2 | 4] -> sampling locations."""
    if ref.shape[-1] == 2:
        norm = torch.tensor([[W, H] for H, W in shapes], dtype=offsets.dtype)
        return ref[:, :, None, :, None, :] + offsets / norm[None, None, None, :, None, :]
    return ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5


def module(sd, c, query, flat, ref, mask=None, dtype=torch.float64, bf16_operands=False, sample=core, parts=False):
    """MSDeformAttn.forward with the weights ``sd`` at ``dtype``; ``sample`` is the operator (core or core_grid_sample)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    query, flat, ref = query.to(dtype), flat.to(dtype), ref.to(dtype)
    N, Lq, d = query.shape
    M, shapes, P = c["heads"], c["shapes"], c["P"]
    L = len(shapes)
    value = operand_linear(flat, sd["value_proj.weight"], sd["value_proj.bias"], bf16_operands)
    if mask is not None:
        value = value.masked_fill(mask[..., None], 0.0)
    value = value.view(N, -1, M, d // M)
    offsets = operand_linear(query, sd["sampling_offsets.weight"], sd["sampling_offsets.bias"], bf16_operands).view(N, Lq, M, L, P, 2)
    logits = operand_linear(query, sd["attention_weights.weight"], sd["attention_weights.bias"], bf16_operands).view(N, Lq, M, L * P)
    w = torch.softmax(logits, -1).view(N, Lq, M, L, P)
    loc = locations(offsets, ref, shapes, P)
    out = operand_linear(sample(value, shapes, loc, w), sd["output_proj.weight"], sd["output_proj.bias"], bf16_operands)
    if parts:
        return out, value, offsets, logits, loc, w
    return out


def module_with_grads(sd, c, query, flat, ref, mask, grad_out, dtype=torch.float64, sample=core):
    """-> (out, {name: gradient}) for the eight parameters, "query" and "input_flatten"."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    q, f = query.to(dtype).clone().requires_grad_(True), flat.to(dtype).clone().requires_grad_(True)
    out = module(sd, c, q, f, ref, mask, dtype=dtype, sample=sample)
    names = list(sd) + ["query", "input_flatten"]
    grads = torch.autograd.grad(out, list(sd.values()) + [q, f], grad_out.to(dtype))
    return out.detach(), dict(zip(names, grads))


def make_core_inputs(c):
    rs = np.random.RandomState(c["seed"])
    M, D, shapes, P, Lq = c["M"], c["D"], c["shapes"], c["P"], c["Lq"]
    L = len(shapes)
    value = torch.from_numpy(rs.standard_normal((N_BATCH, pixels(shapes), M, D)).astype(np.float32))
    loc = draw_locations(rs, N_BATCH, Lq, M, shapes, P)
    w = torch.softmax(torch.from_numpy(rs.standard_normal((N_BATCH, Lq, M, L * P)).astype(np.float32)), -1).view(N_BATCH, Lq, M, L, P)
    grad_out = torch.from_numpy(rs.standard_normal((N_BATCH, Lq, M * D)).astype(np.float32))
    return value, loc, w, grad_out


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
