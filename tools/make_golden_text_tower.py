"""Writes tests/golden/f18_text_tower.npz: outputs of HF ``transformers.SiglipTextModel`` (fp32, CPU, eager attention) on two small
configurations, with and without a key-padding mask.  Run once, by hand, where ``transformers`` is installed:

    python tools/make_golden_text_tower.py

The weights are NOT stored (the wider configuration has 2.9 M of them): the fixture records each configuration's seed and
``tests/text_tower_oracle.make_weights`` redraws them from ``numpy.random.RandomState`` here and in the tests.  Stored per
configuration ``<name>``: ``<name>.seed``, ``<name>.ids`` [3, 16], ``<name>.mask`` (valid lengths 16, 5, 1, right-padded),
``<name>.mask_last`` (the last position masked), and ``<name>.<case>.last_hidden_state`` / ``.pooler_output`` for ``<case>`` in
``nomask``, ``mask``, ``mask_last``.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import text_tower_oracle as TO  # noqa: E402


def hf_model(cfg, sd):
    from transformers import SiglipTextConfig, SiglipTextModel
    m = SiglipTextModel(SiglipTextConfig(attn_implementation="eager", **cfg)).eval()
    own = m.state_dict()
    prefix = "text_model." if any(k.startswith("text_model.") for k in own) else ""
    missing, unexpected = m.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


def main():
    out = {}
    for name, cfg in TO.CONFIGS.items():
        seed = TO.SEEDS[name]
        sd = TO.make_weights(cfg, seed)
        ids, mask, mask_last = TO.make_ids_and_masks(cfg, seed)
        m = hf_model(cfg, sd)
        out[f"{name}.seed"] = np.int64(seed)
        out[f"{name}.ids"] = ids.numpy()
        out[f"{name}.mask"] = mask.numpy()
        out[f"{name}.mask_last"] = mask_last.numpy()
        for case, am in (("nomask", None), ("mask", mask), ("mask_last", mask_last)):
            with torch.no_grad():
                r = m(input_ids=ids, attention_mask=am)
            out[f"{name}.{case}.last_hidden_state"] = r.last_hidden_state.numpy().astype(np.float32)
            out[f"{name}.{case}.pooler_output"] = r.pooler_output.numpy().astype(np.float32)
            want = TO.forward(sd, cfg, ids, am)
            print(f"{name} {case}: HF fp32 against the fp64 restatement: last {float((r.last_hidden_state.double() - want[0]).abs().max()):.2e} "
                  f"pooled {float((r.pooler_output.double() - want[1]).abs().max()):.2e}  (max |pooled| {float(want[1].abs().max()):.2f})")
    path = TO.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
