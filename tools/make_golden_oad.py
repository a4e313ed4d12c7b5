"""Fixture F20 (tests/golden/f20_oad.npz): the reference's own LSTRStream.stream_inference, fp64 on the CPU, on two small detectors.

    python tools/make_golden_oad.py /path/to/reference/downstream/OAD/src

The reference package is imported from the path argument (never on the GPU machine; nothing of it is stored).  ``cfg`` is built from
``types.SimpleNamespace`` with the fields LSTR.__init__ reads; the feature width of each case is added to the reference's FEATURE_SIZES
dict at run time.  Stored per case: the SEED of the weights (0.67 M of them per case, 2.7 MB: tests/oad_oracle.make_weights redraws them from
numpy.random.RandomState, whose streams are frozen across NumPy versions, here and in the tests alike, as fixture F18 does), the list of
ALL state-dict keys of the reference model, the inputs and the scores of every step.

Each case: 32 steps of one stream.  Step 0 passes the whole long window with its 5 oldest slots masked -inf; every 2nd step after it
passes one new long sample, so the ring wraps (16 pushes against L = 12 / 8); the mask shrinks by one slot per push, the data layer's rule.
"""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import oad_oracle as OO      # noqa: E402

STEPS, MASKED, SEEDS = 32, 5, {"a": 2001, "b": 2002}


def reference_cfg(c, feature):
    lstr = NS(LONG_MEMORY_NUM_SAMPLES=c["long_samples"], WORK_MEMORY_NUM_SAMPLES=c["work_samples"], ANTICIPATION_NUM_SAMPLES=0,
              FUTURE_NUM_SAMPLES=0, NUM_HEADS=c["heads"], DIM_FEEDFORWARD=c["ffn"], DROPOUT=0.2, ACTIVATION=c["activation"],
              ENC_MODULE=c["enc_module"], DEC_MODULE=c["dec_module"], GROUPS=0)
    return NS(MODEL=NS(MODEL_NAME="LSTR", LSTR=lstr,
                       FEATURE_HEAD=NS(LINEAR_ENABLED=c["linear_enabled"], LINEAR_OUT_FEATURES=c["d_model"] if c["linear_enabled"] else -1)),
              DATA=NS(NUM_CLASSES=c["classes"], DATA_NAME="THUMOS"), INPUT=NS(MODALITY="visual", VISUAL_FEATURE=feature, MOTION_FEATURE=feature))


def main():
    sys.path.insert(0, sys.argv[1])
    from rekognition_online_action_detection.models import feature_head, lstr
    out = {}
    for name, c in OO.CASES.items():
        feature = f"f20_{name}"
        feature_head.FEATURE_SIZES[feature] = c["d_in"]
        model = lstr.LSTRStream(reference_cfg(c, feature)).double().eval()
        sd = OO.make_weights(c, SEEDS[name])
        keys = list(model.state_dict().keys())
        assert set(keys) == set(sd) | {"pos_encoding.pe"}, sorted(set(keys) ^ set(sd))
        res = model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
        assert res.missing_keys == ["pos_encoding.pe"] and not res.unexpected_keys
        L, W = c["long_samples"], c["work_samples"]
        rs = np.random.RandomState(SEEDS[name] + 5)
        work = rs.standard_normal((STEPS, W, c["d_in"]))
        longs = rs.standard_normal((STEPS, c["d_in"]))
        window = rs.standard_normal((L, c["d_in"]))
        masks = np.zeros((STEPS, L))
        has_long = np.zeros(STEPS, dtype=np.int64)
        scores = np.zeros((STEPS, W, c["classes"]))
        pushes = 0
        with torch.no_grad():
            for t in range(STEPS):
                lg = None
                if t == 0:
                    lg = torch.from_numpy(window)[None]
                elif t % 2 == 1:
                    lg = torch.from_numpy(longs[t:t + 1])[None]
                    pushes += 1
                masks[t, :max(0, MASKED - pushes)] = float("-inf")
                has_long[t] = lg is not None
                motion = None if lg is None else torch.zeros(1, lg.shape[1], 1, dtype=torch.float64)
                wk = torch.from_numpy(work[t])[None]
                y = model.stream_inference(lg, motion, wk, torch.zeros(1, W, 1, dtype=torch.float64), torch.from_numpy(masks[t])[None])
                scores[t] = y[0].numpy()
        assert pushes > L and np.isfinite(scores).all()
        out[f"{name}.seed"] = np.array(SEEDS[name])
        out[f"{name}.keys"] = np.array(keys)
        out[f"{name}.work"], out[f"{name}.long"], out[f"{name}.long_window"] = work, longs, window
        out[f"{name}.mask"], out[f"{name}.has_long"], out[f"{name}.scores"] = masks, has_long, scores
        print(name, "steps", STEPS, "pushes", pushes, "max |score|", float(np.abs(scores).max()))
    path = OO.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
