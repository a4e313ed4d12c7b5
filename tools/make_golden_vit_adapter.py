"""Fixture F22 (tests/golden/f22_vit_adapter.npz): the reference's own ``TimesformerMultiTaskingModelSigLIPViTAdapter`` in fp64 on the CPU,
in ``eval()`` (its SyncBatchNorm layers then apply their running statistics).

    python tools/make_golden_vit_adapter.py /path/to/reference

The path argument goes on sys.path (never on the GPU machine; nothing of the reference is stored).  ``transformers`` is imported first;
then stand-ins are registered for what ``models.modeling_timesformer_siglip_adapter`` imports but does not need for this forward:
``timm.models.layers`` (``DropPath`` as identity, ``trunc_normal_`` = torch's), an EMPTY ``MultiScaleDeformableAttention`` (the compiled
extension: without it ``MSDeformAttn.forward`` takes its own CPU path, ms_deform_attn_core_pytorch), and the package path
``downstream.OVIS.mask2former.modeling.pixel_decoder`` as bare namespace modules pointing at the reference's directories, so that the
real ``ops`` package is imported while the ``__init__`` files above it, which pull in detectron2, never run.

The reference's embeddings take a non-square input (they resize the position table), so the ``rect`` case is kept.  Its two interaction
blocks run only with ``add_vit_feature=False``: the reference's forward unpacks exactly four kept ViT maps otherwise (adapter:661).

Stored per case of tests/vit_adapter_oracle.CASES: the SEED of the weights (vit_adapter_oracle.make_weights redraws them), ALL
state-dict keys of the reference module in its order, the input (values fp16 holds exactly, stored as fp16), the four outputs in fp64
and ``c`` after every interaction block in fp64.  No weights.  Every array is a pure function of the seeds: a second run writes the same
bytes.  fp64 arrays do not compress, so the fixture is kept in parts of at most 1 MiB each (vit_adapter_oracle.golden_files): the main file
with seeds, keys, inputs and res3..res5 of every case, and per case one file for res2 and one for the ``c`` tensors.
"""
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vit_adapter_oracle as VO      # noqa: E402


def _stub_imports(ref_root):
    import transformers  # noqa: F401  (first: it probes for timm and must not find the stand-in half-built)
    layers = types.ModuleType("timm.models.layers")
    layers.DropPath = lambda *a, **k: torch.nn.Identity()
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    for name in ("timm", "timm.models"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
            sys.modules[name] = m
    sys.modules["timm.models.layers"] = layers
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    path = ref_root
    for i, part in enumerate(("downstream", "OVIS", "mask2former", "modeling", "pixel_decoder")):
        path = os.path.join(path, part)
        name = ".".join(("downstream", "OVIS", "mask2former", "modeling", "pixel_decoder")[:i + 1])
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    sys.path.insert(0, ref_root)


def main():
    _stub_imports(os.path.abspath(sys.argv[1]))
    from models.configuration_streamformer import StreamformerConfig
    from models.modeling_timesformer_siglip_adapter import TimesformerMultiTaskingModelSigLIPViTAdapter, deform_inputs
    out = {}
    for name, c in VO.CASES.items():
        cfg = StreamformerConfig(**{k: v for k, v in VO.config(c).to_dict().items() if k != "model_type"})
        torch.manual_seed(c["seed"])
        model = TimesformerMultiTaskingModelSigLIPViTAdapter(cfg, **VO.adapter_kwargs(c))
        ref_sd = model.state_dict()
        sd = VO.make_weights(c)
        assert list(sd) != [] and set(sd) == set(ref_sd), sorted(set(sd) ^ set(ref_sd))
        for k, v in ref_sd.items():
            assert tuple(v.shape) == tuple(sd[k].shape), (k, tuple(v.shape), tuple(sd[k].shape))
        model = model.double().eval()
        model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
        pixels = VO.make_pixels(c)
        cs = []
        hooks = [blk.register_forward_hook(lambda m, a, o: cs.append(o[1].detach())) for blk in model.interactions]
        with torch.no_grad():
            res = model(pixels.double())
        for h in hooks:
            h.remove()
        assert list(res) == list(VO.OUTPUTS) and len(cs) == len(c["indexes"])
        d1, d2 = deform_inputs(pixels.reshape(-1, *pixels.shape[2:]))
        assert torch.equal(d2[0], VO.reference_points(VO.level_shapes(*VO.grid(c)))), "the oracle's reference points differ from the reference's"
        out[f"{name}.seed"] = np.int64(c["seed"])
        out[f"{name}.keys"] = np.array(list(ref_sd.keys()))
        out[f"{name}.pixels"] = pixels.numpy().astype(np.float16)
        assert np.array_equal(out[f"{name}.pixels"].astype(np.float32), pixels.numpy())
        for k in VO.OUTPUTS:
            out[f"{name}.{k}"] = res[k].numpy()
        for i, t in enumerate(cs):
            out[f"{name}.c{i}"] = t.numpy()
        print(f"{name}: " + ", ".join(f"{k} {tuple(res[k].shape)} max {float(res[k].abs().max()):.3f}" for k in VO.OUTPUTS))
    for path, keys in VO.golden_files(out).items():
        np.savez_compressed(path, **{k: out[k] for k in keys})
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 1 << 20, "a fixture file above 1 MiB"


if __name__ == "__main__":
    main()
