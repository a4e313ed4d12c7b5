"""Fixture F23 (tests/golden/f23_pixel_decoder.npz): the reference's own ``MSDeformAttnPixelDecoder`` in fp64 on the CPU, in ``eval()``.

    python tools/make_golden_pixel_decoder.py /path/to/reference

The path argument goes on sys.path (never on the GPU machine; nothing of the reference is stored).  detectron2 and fvcore are not needed:
stand-ins written from the reference's call sites are registered for ``detectron2.config.configurable`` (identity),
``detectron2.layers.{Conv2d, ShapeSpec, get_norm}``, ``detectron2.modeling.SEM_SEG_HEADS_REGISTRY``, ``fvcore.nn.weight_init``, an EMPTY
``MultiScaleDeformableAttention`` (the compiled extension: without it ``MSDeformAttn.forward`` takes its own CPU path), and the packages
above ``pixel_decoder/`` and ``transformer_decoder/`` as bare namespace modules pointing at the reference's directories, so that their
detectron2-importing ``__init__`` files never run.

Two properties of the reference shape the fixture.  ``forward_features`` casts every input with ``.float()``, which a double model then
refuses, so the inputs are passed as a Tensor subclass whose ``float()`` returns itself.  ``PositionEmbeddingSine`` and
``get_reference_points`` compute in fp32 whatever the model's dtype is; that stays in the fixture, and tests/pixel_decoder_oracle.py
restates it under ``table="as_reference"``.

Stored per case of tests/pixel_decoder_oracle.CASES: the SEED of the weights (``make_weights`` redraws them), ALL state-dict keys of the
reference module in its order, the inputs (values fp16 holds exactly, stored as fp16), ``mask_features`` and the first three entries of
``out`` in fp64.  No weights.  Every array is a pure function of the seeds: a second run writes the same bytes.
"""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pixel_decoder_oracle as PO      # noqa: E402

PKG = ("downstream", "OVIS", "mask2former", "modeling")


class _KeepsDtype(torch.Tensor):
    """A tensor whose ``float()`` is itself: the reference's ``features[f].float()`` then leaves a double input double."""

    def float(self, *a, **k):
        return self


class _Conv2d(torch.nn.Conv2d):
    """What the reference's call sites need of detectron2's wrapper: ``norm`` and ``activation`` applied after the convolution."""

    def __init__(self, *args, norm=None, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.norm, self.activation = norm, activation

    def forward(self, x):
        x = super().forward(x)
        if self.norm is not None:
            x = self.norm(x)
        return x if self.activation is None else self.activation(x)


class _ShapeSpec:
    def __init__(self, channels=None, stride=None):
        self.channels, self.stride = channels, stride


class _Registry:
    def register(self, obj=None):
        return obj if obj is not None else (lambda o: o)


def _get_norm(norm, channels):
    if norm in (None, ""):
        return None
    assert norm == "GN", norm
    return torch.nn.GroupNorm(32, channels)


def _c2_xavier_fill(module):
    torch.nn.init.kaiming_uniform_(module.weight, a=1)
    if module.bias is not None:
        torch.nn.init.constant_(module.bias, 0)


def _module(name, package=False, path=None, **attrs):
    m = types.ModuleType(name)
    if package:
        m.__path__ = [path] if path else []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _stub_imports(ref_root):
    _module("detectron2", package=True)
    _module("detectron2.config", configurable=lambda f=None, **k: f if f is not None else (lambda g: g))
    _module("detectron2.layers", Conv2d=_Conv2d, ShapeSpec=_ShapeSpec, get_norm=_get_norm)
    _module("detectron2.modeling", SEM_SEG_HEADS_REGISTRY=_Registry())
    _module("fvcore", package=True)
    _module("fvcore.nn", package=True)
    sys.modules["fvcore.nn"].weight_init = _module("fvcore.nn.weight_init", c2_xavier_fill=_c2_xavier_fill)
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    path = ref_root
    for i, part in enumerate(PKG):
        path = os.path.join(path, part)
        _module(".".join(PKG[:i + 1]), package=True, path=path)
    for leaf in ("pixel_decoder", "transformer_decoder"):
        _module(".".join(PKG + (leaf,)), package=True, path=os.path.join(path, leaf))
    sys.path.insert(0, ref_root)


def main():
    _stub_imports(os.path.abspath(sys.argv[1]))
    ref = importlib.import_module(".".join(PKG + ("pixel_decoder", "msdeformattn")))
    out = {}
    for name, c in PO.CASES.items():
        torch.manual_seed(c["seed"])
        shape = {k: _ShapeSpec(channels=ch, stride=s) for k, ch, s in zip(PO.LEVELS, c["channels"], PO.STRIDES)}
        model = ref.MSDeformAttnPixelDecoder(shape, **PO.decoder_kwargs(c))
        ref_sd = model.state_dict()
        sd = PO.make_weights(c)
        assert list(sd) == list(ref_sd), [(a, b) for a, b in zip(sd, ref_sd) if a != b][:4]
        for k, v in ref_sd.items():
            assert tuple(v.shape) == tuple(sd[k].shape), (k, tuple(v.shape), tuple(sd[k].shape))
        model = model.double().eval()
        model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        feats = PO.make_features(c)
        with torch.no_grad():
            mask, first, ms = model.forward_features({k: v.double().as_subclass(_KeepsDtype) for k, v in feats.items()})
        mask, ms = mask.as_subclass(torch.Tensor), [t.as_subclass(torch.Tensor) for t in ms]
        assert mask.dtype == torch.float64 and len(ms) == 3 and torch.equal(first.as_subclass(torch.Tensor), ms[0])
        assert [tuple(t.shape[2:]) for t in ms] == [c["grids"][l] for l in PO.out_levels(c)[:3]]
        out[f"{name}.seed"] = np.int64(c["seed"])
        out[f"{name}.keys"] = np.array(list(ref_sd.keys()))
        out[f"{name}.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
        for k, v in feats.items():
            out[f"{name}.{k}"] = v.numpy().astype(np.float16)
            assert np.array_equal(out[f"{name}.{k}"].astype(np.float32), v.numpy())
        out[f"{name}.mask_features"] = mask.numpy()
        for i, t in enumerate(ms):
            out[f"{name}.out{i}"] = t.numpy()
        print(f"{name}: mask_features {tuple(mask.shape)} max {float(mask.abs().max()):.3f}, " +
              ", ".join(f"out{i} {tuple(t.shape)}" for i, t in enumerate(ms)))
    os.makedirs(os.path.dirname(PO.GOLDEN), exist_ok=True)
    np.savez_compressed(PO.GOLDEN, **out)
    print(PO.GOLDEN, os.path.getsize(PO.GOLDEN), "bytes")
    assert os.path.getsize(PO.GOLDEN) <= 1 << 20, "a fixture file above 1 MiB"


if __name__ == "__main__":
    main()
