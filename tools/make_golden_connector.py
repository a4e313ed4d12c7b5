"""Writes tests/golden/f19_connector.npz: fp32 outputs of the reference's OWN connector code (``build_vision_projector``,
``LlavaMetaForCausalLM.get_2dPool`` / ``add_token_per_grid`` / ``add_token_per_frame`` and the video branch of
``prepare_inputs_labels_for_multimodal``, llava_arch:339-390) on the eight tiny configurations of ``tests/connector_oracle.CASES``.
Run once, by hand, with the reference checkout next to this repository or named on the command line:

    python tools/make_golden_connector.py [path/to/reference]

The LLaVA package does not import as a whole without its language models and resamplers, so stub modules stand in for ``llava``,
``llava.model`` (with ``__path__`` set, so that the two real submodules import from their files) and for the resampler / encoder builders
(empty ``build_*`` names); ``llava.model.multimodal_projector.builder`` and ``llava.model.llava_arch`` are then the reference's files.

Stored: ``w.<projector>.<key>`` (the two weight sets, shared by the cases), ``w.<projector>.seed``, and per case ``<name>.features``
[2, P * P, 64] and ``<name>.output`` [tokens, 128].  Data only.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import connector_oracle as CO  # noqa: E402


def import_reference(ref_root):
    base = os.path.join(ref_root, "downstream", "VideoQA", "llava")
    for name, path in (("llava", base), ("llava.model", os.path.join(base, "model"))):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    for name, fn in (("llava.model.multimodal_resampler.builder", "build_vision_resampler"),
                     ("llava.model.multimodal_encoder.builder", "build_vision_tower")):
        m = types.ModuleType(name)
        setattr(m, fn, None)
        sys.modules[name] = m
    import llava.model.llava_arch as arch
    import llava.model.multimodal_projector.builder as builder
    return arch, builder


class _Tower:
    def __init__(self, P):
        self.num_patches_per_side = P


def reference_output(arch, builder, cfg, sd, feats, P):
    config = types.SimpleNamespace(**cfg)
    projector = builder.build_vision_projector(config).eval()
    prefix = "mm_projector."
    projector.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)

    class Tail(arch.LlavaMetaForCausalLM):
        def __init__(self):
            self.config = config
            self.model = types.SimpleNamespace(image_newline=sd["image_newline"])
            self._tower = _Tower(P)

        def get_model(self):
            return self.model

        def get_vision_tower(self):
            return self._tower

    tail = Tail()
    with torch.no_grad():
        x = projector(feats)                                                  # llava_arch:213
        x = tail.get_2dPool(x, cfg["mm_spatial_pool_stride"])                # :330
        pos, merge = cfg["mm_newline_position"], cfg["mm_patch_merge_type"]      # :351-390
        if pos == "grid":
            x = tail.add_token_per_grid(x)
        elif pos == "frame":
            x = tail.add_token_per_frame(x).flatten(0, 1)
        elif pos == "one_token":
            x = x.flatten(0, 1)
            if "unpad" in merge:
                x = torch.cat((x, sd["image_newline"][None]), dim=0)
        else:
            x = x.flatten(0, 1)
    return x.contiguous()


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    arch, builder = import_reference(ref_root)
    out = {}
    weights = {}
    for proj, seed in CO.WEIGHT_SEEDS.items():
        weights[proj] = CO.make_weights(proj, seed)
        out[f"w.{proj}.seed"] = np.int64(seed)
        for k, v in weights[proj].items():
            out[f"w.{proj}.{k}"] = v.numpy()
    for i, (name, (proj, mode, P, newline)) in enumerate(CO.CASES.items()):
        cfg = CO.case_config(name)
        feats = CO.make_features(1910 + i, CO.FRAMES, P)
        got = reference_output(arch, builder, cfg, weights[proj], feats, P)
        out[f"{name}.features"] = feats.numpy()
        out[f"{name}.output"] = got.numpy().astype(np.float32)
        want = CO.forward(weights[proj], cfg, feats)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        print(f"{name}: {tuple(got.shape)}  reference fp32 against the fp64 restatement {float((got.double() - want).abs().max()):.2e}")
    np.savez_compressed(CO.GOLDEN, **out)
    print(CO.GOLDEN, os.path.getsize(CO.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
