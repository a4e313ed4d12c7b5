"""Helper of the ViT-Adapter training tests (not a test file): the training restatement of tests/vit_adapter_oracle.py, its autograd run
with every trainable tensor a leaf, and what that run is asked to satisfy before a gradient is compared against it.

The restatement reuses ``VO.encoder_layer``, ``VO.extractor``, ``VO.dwconv``, ``VO.make_weights`` and the cases, with plain operands
(torch Linears and the restated sampling: the operator sequence of the module's training path).  What differs from ``VO.forward`` is what
``.train()`` changes in the reference: the BatchNorms of the spatial prior module and the four final norms use BATCH statistics (biased
variance) and move their running statistics (momentum 0.1, unbiased variance, ``num_batches_tracked`` + 1), and the frozen backbone
(``freeze_backbone=True``) is run without a graph.  The six pre-ReLU tensors of the spatial prior and the input of its max-pool are recorded.

PIXEL_SEEDS: a ReLU whose pre-activation is within rounding of zero flips its gradient discretely, and so does a max-pool window whose
two largest values are within rounding of each other.  tests/test_vit_adapter_train_cpu.py asserts that NONE of either kind is undecided in
the fp64 oracle; a case whose own pixel seed failed that was searched upwards from seed + 1 on the CPU and the first passing seed is
recorded here (None: the case's own pixels, ``VO.make_pixels``).
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import streamformer_oracle as O
from tests import msda_oracle as MO
from tests import vit_adapter_oracle as VO
from tests.helpers import EPS32, MARGIN, maxabs
from tests.oracle_ops import operand_linear

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOMENTUM = 0.1
# own seeds 2201 / 2202 / 2203 leave (ReLUs inside the band, sign flips, pool ties, moved winners) = (1, 0, 1, 0) / (4, 1, 1, 0) / (2, 0, 0, 0)
PIXEL_SEEDS = {"sq": 2213, "rect": 2468, "novit": 2207}
BACKBONE = ("embeddings.", "encoder.", "post_layernorm.")


def golden_path(name):
    return os.path.join(GOLDEN_DIR, f"f27_vit_adapter_train_{name}.npz")


def weights(name):
    return VO.make_weights(VO.CASES[name])


def pixels(name, seed=None):
    seed = PIXEL_SEEDS[name] if seed is None else seed
    return VO.make_pixels(VO.CASES[name], seed)


def trainable_keys(sd):
    """The parameters ``.train()`` learns: everything floating that is neither the backbone's nor a BatchNorm buffer."""
    return [k for k, v in sd.items() if v.is_floating_point() and not k.startswith(BACKBONE) and not k.endswith((".running_mean", ".running_var"))]


def small(key):
    """Whether a gradient is stored in the fixture in full (the others as a max-abs and two projections)."""
    return key == "level_embed" or "norm" in key or ".dwconv." in key or key.startswith(("spm.stem.1", "spm.stem.4", "spm.stem.7")) or \
        (key.startswith("spm.conv") and ".1." in key)


def cotangents(name, outs):
    """One fixed random cotangent per output res2..res5, fp64 on the CPU."""
    rs = np.random.RandomState(VO.CASES[name]["seed"] + 99)
    return [torch.from_numpy(rs.standard_normal(tuple(outs[k].shape))) for k in VO.OUTPUTS]


def pairing(outs, cots, dtype, device=None):
    total = 0.0
    for k, ct in zip(VO.OUTPUTS, cots):
        total = total + (outs[k] * ct.to(dtype=dtype, device=device or outs[k].device)).sum()
    return total


def projections(name, index, grad):
    """(max-abs, the projections onto two seeded standard-normal vectors) of a gradient, as the fixture stores them."""
    rs = np.random.RandomState(VO.CASES[name]["seed"] + 1000 + index)
    g = grad.detach().double().reshape(-1).numpy()
    return np.array([np.abs(g).max(), g @ rs.standard_normal(g.size), g @ rs.standard_normal(g.size)])


class Run:
    """One run of the training restatement: ``outs`` (res2..res5), ``c`` (the extractors' final tokens), ``stats`` (the moved running
    statistics by state-dict key), the recorded pre-ReLU tensors ``pre`` and the max-pool input ``pool_in``, and (after ``backward``) the
    gradients by state-dict key.

    ``encoder_operands`` is ``VO.forward``'s ``operands`` for the frozen encoder alone (no graph, the library's inference kernels): "x3" in a
    fp32 run makes that run the PRECISION FLOOR of the GPU tests as tests/test_vit_adapter.py defines it for the same kernels (bf16 hi + lo
    planes, three products); everything under autograd keeps plain fp32 operands, which is what the training path runs."""

    def __init__(self, name, dtype, sd=None, px=None, grad=True, encoder_operands=False):
        self.encoder_operands = encoder_operands
        c = self.case = VO.CASES[name]
        sd = weights(name) if sd is None else sd
        px = pixels(name) if px is None else px
        learned = set(trainable_keys(sd))
        self.sd = OrderedDict((k, (v.detach().clone().to(dtype).requires_grad_(grad and k in learned) if v.is_floating_point() else v.clone())) for k, v in sd.items())
        self.pre, self.stats = [], OrderedDict()
        with torch.set_grad_enabled(grad):
            self.outs, self.c = self._forward(c, px.to(dtype))

    def _bn(self, x, p):
        sd = self.sd
        mean, var = sd[p + ".running_mean"].detach().clone(), sd[p + ".running_var"].detach().clone()
        y = F.batch_norm(x, mean, var, sd[p + ".weight"], sd[p + ".bias"], True, MOMENTUM, VO.BN_EPS)
        self.stats[p + ".running_mean"], self.stats[p + ".running_var"] = mean, var
        self.stats[p + ".num_batches_tracked"] = sd[p + ".num_batches_tracked"] + 1
        return y

    def _spatial_prior(self, x):
        sd = self.sd

        def block(x, conv, norm, stride):
            z = self._bn(F.conv2d(x, sd[conv + ".weight"], None, stride, 1), norm)
            self.pre.append(z.detach())
            return F.relu(z)
        c1 = block(x, "spm.stem.0", "spm.stem.1", 2)
        c1 = block(c1, "spm.stem.3", "spm.stem.4", 1)
        c1 = block(c1, "spm.stem.6", "spm.stem.7", 1)
        self.pool_in = c1.detach()
        c1 = F.max_pool2d(c1, 3, 2, 1)
        c2 = block(c1, "spm.conv2.0", "spm.conv2.1", 2)
        c3 = block(c2, "spm.conv3.0", "spm.conv3.1", 2)
        c4 = block(c3, "spm.conv4.0", "spm.conv4.1", 2)
        fc = [F.conv2d(t, sd[f"spm.fc{i + 1}.weight"], sd[f"spm.fc{i + 1}.bias"]) for i, t in enumerate((c1, c2, c3, c4))]
        return (fc[0],) + tuple(t.flatten(2).transpose(1, 2) for t in fc[1:])

    def _forward(self, c, px):
        sd, cfg = self.sd, VO.config(c)
        lin = lambda x, w, b: operand_linear(x, w, b, False)                      # noqa: E731
        enc_lin = lambda x, w, b: operand_linear(x, w, b, self.encoder_operands)  # noqa: E731
        B, T, _, H, W = px.shape
        Fr, D, (Hg, Wg) = B * T, cfg.hidden_size, (H // 16, W // 16)
        n = (Hg // 2) * (Wg // 2)
        c1, c2, c3, c4 = self._spatial_prior(px.reshape(Fr, 3, H, W))
        le = sd["level_embed"]
        cc = torch.cat([c2 + le[0], c3 + le[1], c4 + le[2]], 1)
        with torch.no_grad():
            w = sd["embeddings.patch_embeddings.projection.weight"]
            h = enc_lin(O.patchify(px, 16), w.reshape(D, -1), sd["embeddings.patch_embeddings.projection.bias"])
            h = h + O.position_embedding(sd, cfg, H, W)[None, None] + O.time_embedding_rows(sd, cfg, 0, T, False)[None, :, None, :]
        ref = VO.reference_points(VO.level_shapes(Hg, Wg))
        maps = []
        for (a, b), block in zip(c["indexes"], VO.extractor_prefixes(c)):
            with torch.no_grad():
                for i in range(a, b + 1):
                    h = VO.encoder_layer(sd, cfg, i, h, enc_lin, lambda t: t)
            feat = h.reshape(Fr, Hg * Wg, D)
            for p in block:
                cc = VO.extractor(sd, p, c, cc, feat, ref, Hg, Wg, cfg.layer_norm_eps, lin, False, MO.core)
            maps.append(VO.tokens_to_map(feat, Hg, Wg))
        m2, m3, m4 = (VO.tokens_to_map(cc[:, :16 * n], 2 * Hg, 2 * Wg), VO.tokens_to_map(cc[:, 16 * n:20 * n], Hg, Wg),
                      VO.tokens_to_map(cc[:, 20 * n:], Hg // 2, Wg // 2))
        m1 = F.conv_transpose2d(m2, sd["up.weight"], sd["up.bias"], 2) + c1
        if c["add_vit_feature"]:
            x1, x2, x3, x4 = maps
            m1 = m1 + F.interpolate(x1, scale_factor=4, mode="bilinear", align_corners=False)
            m2 = m2 + F.interpolate(x2, scale_factor=2, mode="bilinear", align_corners=False)
            m3 = m3 + x3
            m4 = m4 + F.interpolate(x4, scale_factor=0.5, mode="bilinear", align_corners=False)
        return OrderedDict((k, self._bn(m, f"norm{i + 1}")) for i, (k, m) in enumerate(zip(VO.OUTPUTS, (m1, m2, m3, m4)))), cc

    def backward(self, cots):
        pairing(self.outs, cots, self.c.dtype).backward()
        return {k: self.sd[k].grad for k in trainable_keys(self.sd)}


def pool_margin(x):
    """Per 3 x 3 / stride 2 / padding 1 window of NCHW ``x``: the largest value minus the second largest (padding never wins)."""
    N, C, H, W = x.shape
    win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")).reshape(N * C, 1, H + 2, W + 2), 3, stride=2)      # [N C, 9, windows]
    top = win.topk(2, dim=1).values
    return top[:, 0] - top[:, 1], win.argmax(dim=1)


def undecided(name, seed=None):
    """-> (ReLU pre-activations inside their band, sign disagreements between the fp32 and the fp64 run, max-pool windows whose top-two
    margin is inside the band, windows whose winner differs between the two runs).  A band is MARGIN times the fp32 floor of the tensor
    it belongs to: what the fp32 run of the same operator sequence loses against fp64, at least one fp32 rounding of the tensor's largest
    magnitude."""
    sd, px = weights(name), pixels(name, seed)
    r64, r32 = Run(name, torch.float64, sd, px, grad=False), Run(name, torch.float32, sd, px, grad=False)
    assert len(r64.pre) == len(r32.pre) == 6
    close = flips = 0
    for a, b in zip(r64.pre, r32.pre):
        band = MARGIN * max(maxabs(b, a), EPS32 * float(a.abs().max()))
        close += int((a.abs() <= band).sum())
        flips += int(((a > 0) != (b > 0)).sum())
    a, b = r64.pool_in, r32.pool_in
    band = MARGIN * max(maxabs(b, a), EPS32 * float(a.abs().max()))
    (m64, w64), (_, w32) = pool_margin(a), pool_margin(b)
    # a tie of two clipped zeros is no tie of gradients: both ReLUs pass nothing
    top = F.max_pool2d(a, 3, 2, 1).reshape(m64.shape)
    ties = int(((m64 <= band) & (top > 0)).sum())
    moved = int(((w64 != w32) & (top > 0)).sum())
    return close, flips, ties, moved


def load_golden(name):
    with np.load(golden_path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_arrays(name, run, grads):
    """What fixture F27 holds for one case, from a fp64 run and its gradients: the same function builds the arrays from the reference's
    class (tools/make_golden_vit_adapter_train.py) and from the restatement (tests/test_vit_adapter_train_cpu.py)."""
    out = OrderedDict()
    out["seed"] = np.int64(VO.CASES[name]["seed"])
    out["pixel_seed"] = np.int64(-1 if PIXEL_SEEDS[name] is None else PIXEL_SEEDS[name])
    out["res2"] = run["outs"]["res2"].detach().numpy()[:, ::4]                       # every fourth channel: the part stays below 1 MiB
    for k in VO.OUTPUTS[1:]:
        out[k] = run["outs"][k].detach().numpy()
    for k, v in run["stats"].items():
        out["stat." + k] = v.detach().numpy()
    keys = sorted(grads)
    out["grad_keys"] = np.array(keys)
    for i, k in enumerate(keys):
        out["grad." + k] = grads[k].detach().numpy() if small(k) else projections(name, i, grads[k])
    return out
