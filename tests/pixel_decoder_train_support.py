"""Helper of the pixel decoder training tests (not a test file): the seeds, the oracle's autograd run with every weight and input a leaf,
and what that run is asked to satisfy before a gradient is compared against it.

The oracle is tests/pixel_decoder_oracle.py's restatement with plain operands (``operands=False``: torch Linears and the restated
sampling, which is the operator sequence of the module's training path) and the fp64 position table.  Its pre-ReLU values (GroupNorm's
ReLU of the FPN outputs, the FFN's ReLU) are recorded by standing in for ``torch.relu`` while it runs.

SEEDS: a ReLU whose pre-activation is within rounding of zero flips its gradient discretely, and so does a bilinear sample whose pixel
coordinate is within rounding of an integer (its location gradient changes corner pairs).  tests/test_pixel_decoder_train_cpu.py asserts
that NONE of either kind is undecided in the fp64 oracle at these seeds; a case whose own seed failed that was searched upwards from
seed + 1 on the CPU and the first passing seed is recorded here.
"""
from collections import OrderedDict
from unittest import mock

import numpy as np
import torch

from tests import pixel_decoder_oracle as PO
from tests.helpers import EPS32, MARGIN, maxabs

FRAMES = 2
SEEDS = {"m2f": None, "all4": None, "res5only": 2304}          # None: the case's own seed; res5only: 2303 leaves two GroupNorm ReLUs undecided


def seed_of(name):
    return PO.CASES[name]["seed"] if SEEDS[name] is None else SEEDS[name]


def weights(name, seed=None):
    return PO.make_weights(PO.CASES[name], seed_of(name) if seed is None else seed)


def features(name, seed=None):
    return PO.make_features(PO.CASES[name], seed_of(name) if seed is None else seed, frames=FRAMES)


def cotangents(name, mask, outs):
    """One fixed random cotangent per output (mask_features, then the three multi-scale features), fp64 on the CPU."""
    rs = np.random.RandomState(PO.CASES[name]["seed"] + 99)
    return [torch.from_numpy(rs.standard_normal(tuple(t.shape))) for t in [mask] + list(outs[:3])]


def pairing(mask, outs, cots, dtype, device=None):
    total = 0.0
    for t, ct in zip([mask] + list(outs[:3]), cots):
        total = total + (t * ct.to(dtype=dtype, device=device or t.device)).sum()
    return total


class Run:
    """One oracle run: outputs, the recorded pre-ReLU tensors and sampling locations, and (after ``backward``) the gradients by name:
    the state-dict keys, and ``x.<level>`` for the inputs."""

    def __init__(self, name, dtype, sd=None, feats=None, grad=True):
        c = PO.CASES[name]
        sd = weights(name) if sd is None else sd
        feats = features(name) if feats is None else feats
        self.sd = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_(grad)) for k, v in sd.items())
        self.feats = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_(grad)) for k, v in feats.items())
        self.pre, self.locations = [], []
        relu = torch.relu

        def recording(t):
            self.pre.append(t.detach())
            return relu(t)

        with mock.patch.object(torch, "relu", recording), torch.set_grad_enabled(grad):
            self.mask, self.out = PO.forward(self.sd, c, self.feats, dtype=dtype, operands=False, table="fp64", locations=self.locations)
        self.locations = [t.detach() for t in self.locations]
        self.shapes = [c["grids"][l] for l in PO.transformer_levels(c)]

    def backward(self, cots):
        pairing(self.mask, self.out, cots, self.mask.dtype).backward()
        grads = {k: v.grad for k, v in self.sd.items()}
        grads.update({f"x.{k}": v.grad for k, v in self.feats.items()})
        return grads

    def pixel_coordinates(self):
        """Per encoder layer the sampling locations in pixels of their level, [N, Lq, M, L, P, 2] of (x, y)."""
        size = torch.tensor([[W, H] for H, W in self.shapes], dtype=self.mask.dtype)
        return [loc * size[None, None, None, :, None, :] - 0.5 for loc in self.locations]


def undecided(name, seed=None):
    """-> (ReLU pre-activations inside their band, sign disagreements between the fp32 and the fp64 run, sample coordinates inside their
    band of an integer, coordinates that round to different integers in the two runs).  A band is MARGIN times the fp32 floor of the
    tensor it belongs to: what the fp32 run of the same operator sequence loses against fp64, at least one fp32 rounding of the tensor's
    largest magnitude."""
    sd, feats = weights(name, seed), features(name, seed)
    r64, r32 = Run(name, torch.float64, sd, feats, grad=False), Run(name, torch.float32, sd, feats, grad=False)
    assert len(r64.pre) == len(r32.pre) and r64.pre
    close = flips = 0
    for a, b in zip(r64.pre, r32.pre):
        band = MARGIN * max(maxabs(b, a), EPS32 * float(a.abs().max()))
        close += int((a.abs() <= band).sum())
        flips += int(((a > 0) != (b > 0)).sum())
    near = moved = 0
    for a, b in zip(r64.pixel_coordinates(), r32.pixel_coordinates()):
        band = MARGIN * max(maxabs(b, a), EPS32 * float(a.abs().max()))
        near += int(((a - a.round()).abs() <= band).sum())
        moved += int((a.floor() != b.double().floor()).sum())
    return close, flips, near, moved
