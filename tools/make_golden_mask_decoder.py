"""Fixture F24 (tests/golden/f24_mask_decoder.npz): the reference's own ``MultiScaleMaskedTransformerDecoder`` and
``CLMultiScaleMaskedTransformerDecoder`` in fp64 on the CPU, in ``eval()``.

    python tools/make_golden_mask_decoder.py /path/to/reference

The path argument goes on sys.path (never on the GPU machine; nothing of the reference is stored).  detectron2 and fvcore are not needed:
stand-ins written from the reference's call sites are registered for ``detectron2.config.configurable`` (identity),
``detectron2.layers.Conv2d``, ``detectron2.structures.BitMasks`` (the box rule: per mask (min x, min y, max x + 1, max y + 1) over its
set pixels, zeros for an empty one, fp32), ``fvcore.nn.weight_init`` and the module that holds ``TRANSFORMER_DECODER_REGISTRY``; the
packages above the two ``transformer_decoder/`` directories are bare namespace modules pointing at the reference's directories, so that
their detectron2-importing ``__init__`` files never run.

``PositionEmbeddingSine`` computes in fp32 whatever the model's dtype is; that stays in the fixture, and tests/mask_decoder_oracle.py
restates it under ``table="as_reference"``.  The attention masks are taken from ``forward_prediction_heads``' return value: the forward
clears fully set rows of that very tensor in place before it uses it, so after the forward it holds what the layer attended under.

Stored per case of tests/mask_decoder_oracle.CASES: the SEED of the weights (``make_weights`` redraws them), ALL state-dict keys of the
reference module in its order and their shapes, the inputs (values fp16 holds exactly, stored as fp16), the output dict in fp64 without
``aux_outputs`` and ``query_pos_embeds`` (a copy of a weight), and every layer's boolean attention mask, bit-packed.  No weights.  Every
array is a pure function of the seeds: a second run writes the same bytes.
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
from tests import mask_decoder_oracle as DO      # noqa: E402

M2F = ("downstream", "OVIS", "mask2former", "modeling", "transformer_decoder")
CTVIS = ("downstream", "OVIS", "ctvis", "modeling", "transformer_decoder")


class _Conv2d(torch.nn.Conv2d):
    def __init__(self, *args, norm=None, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        assert norm is None and activation is None


class _Boxes:
    def __init__(self, tensor):
        self.tensor = tensor

    def to(self, device):
        return _Boxes(self.tensor.to(device))


class _BitMasks:
    def __init__(self, tensor):
        self.tensor = tensor.to(torch.bool)

    def get_bounding_boxes(self):
        boxes = torch.zeros(self.tensor.shape[0], 4, dtype=torch.float32)
        x_any, y_any = torch.any(self.tensor, dim=1), torch.any(self.tensor, dim=2)
        for i in range(self.tensor.shape[0]):
            x, y = torch.where(x_any[i])[0], torch.where(y_any[i])[0]
            if len(x) > 0 and len(y) > 0:
                boxes[i] = torch.as_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1], dtype=torch.float32)
        return _Boxes(boxes)


class _Registry:
    def register(self, obj=None):
        return obj if obj is not None else (lambda o: o)


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
    _module("detectron2.layers", Conv2d=_Conv2d)
    _module("detectron2.structures", BitMasks=_BitMasks)
    _module("fvcore", package=True)
    _module("fvcore.nn", package=True)
    sys.modules["fvcore.nn"].weight_init = _module("fvcore.nn.weight_init", c2_xavier_fill=_c2_xavier_fill)
    for pkg in (M2F, CTVIS):
        path = ref_root
        for i, part in enumerate(pkg):
            path = os.path.join(path, part)
            if ".".join(pkg[:i + 1]) not in sys.modules:
                _module(".".join(pkg[:i + 1]), package=True, path=path)
    _module(".".join(M2F + ("maskformer_transformer_decoder",)), TRANSFORMER_DECODER_REGISTRY=_Registry())
    sys.path.insert(0, ref_root)


def main():
    _stub_imports(os.path.abspath(sys.argv[1]))
    classes = {"MultiScaleMaskedTransformerDecoder": importlib.import_module(".".join(M2F + ("mask2former_transformer_decoder",))),
               "CLMultiScaleMaskedTransformerDecoder": importlib.import_module(".".join(CTVIS + ("cl_mask2former_transformer_decoder",)))}
    out = {}
    for name, c in DO.CASES.items():
        torch.manual_seed(c["seed"])
        model = getattr(classes[c["cls"]], c["cls"])(c["in_channels"], **DO.decoder_kwargs(c))
        ref_sd = model.state_dict()
        sd = DO.make_weights(c)
        assert list(sd) == list(ref_sd), [(a, b) for a, b in zip(sd, ref_sd) if a != b][:4]
        for k, v in ref_sd.items():
            assert tuple(v.shape) == tuple(sd[k].shape), (k, tuple(v.shape), tuple(sd[k].shape))
        model = model.double().eval()
        model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        recorded = []
        heads = model.forward_prediction_heads

        def recording(*a, _heads=heads, **k):
            r = _heads(*a, **k)
            recorded.append(r[2])
            return r

        model.forward_prediction_heads = recording
        xs, mf = DO.make_inputs(c)
        with torch.no_grad():
            res = model([x.double() for x in xs], mf.double())
        assert len(recorded) == c["layers"] + 1 and len(res["aux_outputs"]) == c["layers"]
        out[f"{name}.seed"] = np.int64(c["seed"])
        out[f"{name}.keys"] = np.array(list(ref_sd.keys()))
        out[f"{name}.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
        for k, v in [(f"x{l}", x) for l, x in enumerate(xs)] + [("mask_features", mf)]:
            out[f"{name}.{k}"] = v.numpy().astype(np.float16)
            assert np.array_equal(out[f"{name}.{k}"].astype(np.float32), v.numpy())
        for k in DO.OUTPUTS:
            if k in res:
                out[f"{name}.{k}"] = res[k].double().numpy()
        for i in range(c["layers"]):
            m = recorded[i]                                  # [F * heads, Q, hw], the heads' copies are equal
            m = m.reshape(mf.shape[0], c["heads"], c["queries"], -1)
            assert bool((m == m[:, :1]).all())
            out[f"{name}.attn_mask{i}"] = DO.pack_mask(m[:, 0].numpy())
        print(f"{name}: pred_masks {tuple(res['pred_masks'].shape)} max {float(res['pred_masks'].abs().max()):.3f}; hidden share per layer " +
              ", ".join(f"{float(recorded[i].double().mean()):.2f}" for i in range(c["layers"])))
    os.makedirs(os.path.dirname(DO.GOLDEN), exist_ok=True)
    np.savez_compressed(DO.GOLDEN, **out)
    print(DO.GOLDEN, os.path.getsize(DO.GOLDEN), "bytes")
    assert os.path.getsize(DO.GOLDEN) <= 1 << 20, "a fixture file above 1 MiB"


if __name__ == "__main__":
    main()
