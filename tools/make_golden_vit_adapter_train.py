"""Fixture F27 (tests/golden/f27_vit_adapter_train_<case>.npz): the reference's own ``TimesformerMultiTaskingModelSigLIPViTAdapter`` in
fp64 on the CPU, in ``train()`` with its default frozen backbone, one forward and one backward of a seeded pairing of the four outputs.

    python tools/make_golden_vit_adapter_train.py /path/to/reference

The path argument goes on sys.path exactly as in tools/make_golden_vit_adapter.py (whose import stand-ins are reused; nothing of the
reference is stored).  ``SyncBatchNorm`` refuses CPU input in training mode, so after construction every instance is swapped for a
``BatchNorm2d`` holding the same tensors: one process, one rank, the same arithmetic.

Stored per case of tests/vit_adapter_oracle.CASES, one file each (fp64 does not compress; every file stays below 1 MiB): the weight seed
and the pixel seed (tests/vit_adapter_train_support.PIXEL_SEEDS; -1: the case's own pixels), res3..res5 and every fourth channel of res2,
the running statistics and batch counts after the step, the sorted names of the trainable parameters and per name its gradient: in full for
the small tensors (level_embed, norms, dwconv weights and biases), otherwise as (max-abs, projection onto two seeded vectors).  No
weights.  tests/vit_adapter_train_support.golden_arrays builds the arrays, here from the reference's class and in
tests/test_vit_adapter_train_cpu.py from the restatement.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_vit_adapter import _stub_imports                # noqa: E402
from tests import vit_adapter_oracle as VO                       # noqa: E402
from tests import vit_adapter_train_support as TS                # noqa: E402


def _plain_batchnorm(module):
    """Every SyncBatchNorm below ``module`` replaced by a BatchNorm2d that holds the same parameters and buffers."""
    for name, child in list(module.named_children()):
        if isinstance(child, torch.nn.SyncBatchNorm):
            bn = torch.nn.BatchNorm2d(child.num_features, child.eps, child.momentum, child.affine, child.track_running_stats)
            bn.weight, bn.bias = child.weight, child.bias
            bn.running_mean, bn.running_var, bn.num_batches_tracked = child.running_mean, child.running_var, child.num_batches_tracked
            setattr(module, name, bn)
        else:
            _plain_batchnorm(child)


def main():
    _stub_imports(os.path.abspath(sys.argv[1]))
    from models.configuration_streamformer import StreamformerConfig
    from models.modeling_timesformer_siglip_adapter import TimesformerMultiTaskingModelSigLIPViTAdapter
    for name, c in VO.CASES.items():
        cfg = StreamformerConfig(**{k: v for k, v in VO.config(c).to_dict().items() if k != "model_type"})
        torch.manual_seed(c["seed"])
        model = TimesformerMultiTaskingModelSigLIPViTAdapter(cfg, **VO.adapter_kwargs(c))
        _plain_batchnorm(model)
        sd = TS.weights(name)
        model = model.double()
        model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        model.train()
        learned = {k for k, p in model.named_parameters() if p.requires_grad}
        assert learned == set(TS.trainable_keys(sd)), sorted(learned ^ set(TS.trainable_keys(sd)))
        outs = model(TS.pixels(name).double())
        assert list(outs) == list(VO.OUTPUTS)
        TS.pairing(outs, TS.cotangents(name, outs), torch.float64).backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
        assert all(g is not None for g in grads.values())
        stats = {k: v for k, v in model.state_dict().items() if k.endswith((".running_mean", ".running_var", ".num_batches_tracked"))}
        arrays = TS.golden_arrays(name, dict(outs=outs, stats=stats), grads)
        path = TS.golden_path(name)
        np.savez_compressed(path, **arrays)
        print(f"{name}: {len(grads)} gradients, " + ", ".join(f"{k} {tuple(outs[k].shape)}" for k in VO.OUTPUTS), path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 1 << 20, "a fixture file above 1 MiB"


if __name__ == "__main__":
    main()
