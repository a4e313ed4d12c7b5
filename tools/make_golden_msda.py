"""Fixture F21 (tests/golden/f21_msda.npz): the reference's own MSDeformAttn and ms_deform_attn_core_pytorch, fp64 on the CPU.

    python tools/make_golden_msda.py /path/to/reference/downstream/OVIS/mask2former/modeling/pixel_decoder

The path argument goes on sys.path and the reference's ``ops`` package is imported from it (never on the GPU machine; nothing of it is
stored).  Its ``ms_deform_attn_func.py`` insists on the compiled extension ``MultiScaleDeformableAttention``: an EMPTY module of that name
is registered first, the import succeeds, and ``MSDeformAttn.forward`` then takes its own CPU path (ms_deform_attn_core_pytorch) when the
extension call fails.

Stored per operator case (tests/msda_oracle.CORE_CASES): value, sampling locations, attention weights and grad_out in fp32, the output and
the three autograd gradients in fp64.  Per module case (MODULE_CASES): the SEED of the weights (tests/msda_oracle.make_weights redraws them
from numpy.random.RandomState, as fixtures F18 and F20 do), ALL state-dict keys of the reference module, its sampling_offsets.bias as
_reset_parameters leaves it, the inputs (values fp16 holds exactly, stored as fp16), the output in fp64 and, for the two small cases, the
autograd gradients of every parameter, of the query and of input_flatten.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import msda_oracle as MO      # noqa: E402


def main():
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    sys.path.insert(0, sys.argv[1])
    from ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch
    from ops.modules import MSDeformAttn
    out = {}
    for name, c in MO.CORE_CASES.items():
        value, loc, w, grad_out = MO.make_core_inputs(c)
        v, l, a = (t.double().requires_grad_(True) for t in (value, loc, w))
        y = ms_deform_attn_core_pytorch(v, c["shapes"], l, a)
        gv, gl, ga = torch.autograd.grad(y, (v, l, a), grad_out.double())
        for k, t in (("value", value), ("loc", loc), ("w", w), ("grad_out", grad_out)):
            out[f"{name}.{k}"] = t.numpy()
        for k, t in (("out", y), ("grad_value", gv), ("grad_loc", gl), ("grad_w", ga)):
            out[f"{name}.{k}"] = t.detach().numpy()
        print(f"{name}: out {tuple(y.shape)}, max |out| {float(y.detach().abs().max()):.3f}")
    for name, c in MO.MODULE_CASES.items():
        shapes = c["shapes"]
        torch.manual_seed(c["seed"])
        model = MSDeformAttn(c["d_model"], len(shapes), c["heads"], c["P"], ratio=0.5)
        out[f"{name}.keys"] = np.array(list(model.state_dict().keys()))
        out[f"{name}.init_offsets_bias"] = model.sampling_offsets.bias.detach().numpy().copy()
        sd = MO.make_weights(c)
        assert set(sd) == set(model.state_dict().keys())
        model = model.double()
        model.load_state_dict({k: v.double() for k, v in sd.items()})
        query, flat, ref, mask, grad_out = MO.make_module_inputs(c)
        q, f = query.double().requires_grad_(True), flat.double().requires_grad_(True)
        y = model(q, ref.double(), f, torch.tensor(shapes), torch.tensor(MO.level_starts(shapes)), mask)
        out[f"{name}.seed"] = np.int64(c["seed"])
        for k, t in (("query", query), ("input_flatten", flat), ("reference_points", ref), ("grad_out", grad_out)):
            out[f"{name}.{k}"] = t.numpy().astype(np.float16)
            assert np.array_equal(out[f"{name}.{k}"].astype(np.float32), t.numpy())
        if mask is not None:
            out[f"{name}.mask"] = mask.numpy()
        out[f"{name}.out"] = y.detach().numpy()
        if c["grads"]:
            assert MO.away_from_integers(MO.module(sd, c, query, flat, ref, mask, parts=True)[4], shapes), "a sample sits on a pixel boundary"
            params = dict(model.named_parameters())
            grads = torch.autograd.grad(y, list(params.values()) + [q, f], grad_out.double())
            for k, g in zip(list(params) + ["query", "input_flatten"], grads):
                out[f"{name}.grad.{k}"] = g.numpy()
        print(f"{name}: out {tuple(y.shape)}, max |out| {float(y.detach().abs().max()):.3f}")
    np.savez_compressed(MO.GOLDEN, **out)
    print(MO.GOLDEN, os.path.getsize(MO.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
