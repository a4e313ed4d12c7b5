"""CPU: the online-action-detection oracle against the reference's stored scores (tests/golden/f20_oad.npz, made by
tools/make_golden_oad.py from the reference's own LSTRStream in fp64), its ring against a from-scratch evaluation, and the host side
of streamformer_amd.oad: configuration, parameter tree, ignored keys and refusals.  No GPU is touched."""
import pytest
import torch

from tests import oad_oracle as OO
from tests.helpers import maxabs

NINF = float("-inf")


@pytest.fixture(scope="module")
def gold():
    return OO.load_golden()


def _config(c, **kw):
    import streamformer_amd as sa
    base = dict(VISUAL_SIZE=c["d_in"], NUM_CLASSES=c["classes"], LINEAR_ENABLED=c["linear_enabled"],
                LINEAR_OUT_FEATURES=c["d_model"] if c["linear_enabled"] else -1, NUM_HEADS=c["heads"], DIM_FEEDFORWARD=c["ffn"],
                ACTIVATION=c["activation"], LONG_MEMORY_NUM_SAMPLES=c["long_samples"], WORK_MEMORY_NUM_SAMPLES=c["work_samples"],
                ENC_MODULE=c["enc_module"], DEC_MODULE=c["dec_module"])
    base.update(kw)
    return sa.OADConfig(**base)


@pytest.mark.parametrize("name", list(OO.CASES))
def test_oracle_reproduces_every_stored_step(gold, name):
    """Bound 1e-9 on scores of O(1); the reference ran in fp64 and the measured gap is 3.6e-15 (a) / 3.4e-15 (b): summation order only."""
    sd, steps = OO.golden_case(gold, name)
    assert len(steps) >= 30 and sum(1 for s in steps[1:] if s[1] is not None) > OO.CASES[name]["long_samples"]
    assert steps[0][1].shape[0] == OO.CASES[name]["long_samples"] and int((steps[0][2] == NINF).sum()) == 5
    st = OO.Stream(sd, OO.CASES[name])
    worst = 0.0
    for work, lg, mk, stored in steps:
        worst = max(worst, maxabs(st.step(work, lg, mk), stored))
    print(f"F20 {name}: oracle against the reference, max-abs {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("name", list(OO.CASES))
def test_oracle_ring_equals_from_scratch(gold, name):
    """The incremental ring result at step t equals the oracle run from scratch on the full last window (fp64: summation order only)."""
    sd, steps = OO.golden_case(gold, name)
    st, scratch = OO.Stream(sd, OO.CASES[name]), OO.Stream(sd, OO.CASES[name])
    window = steps[0][1]
    checked = 0
    for t, (work, lg, mk, _) in enumerate(steps):
        y = st.step(work, lg, mk)
        if lg is None:
            continue
        if t:
            window = torch.cat([window[1:], lg])
        assert maxabs(scratch.from_scratch(work, window, mk), y) <= 1e-12, t
        checked += 1
    assert checked > OO.CASES[name]["long_samples"]


def test_config_validation_and_round_trip():
    import streamformer_amd as sa
    c = OO.CASES["a"]
    cfg = _config(c)
    assert cfg.d_model == 128 and _config(OO.CASES["b"]).d_model == 128
    again = sa.OADConfig.from_reference_dict(cfg.to_reference_dict())
    assert again == cfg
    thumos = {"INPUT": {"MODALITY": "visual", "VISUAL_FEATURE": "streamformer_multitask_feature"}, "DATA": {"DATA_NAME": "THUMOS", "NUM_CLASSES": 22},
              "MODEL": {"FEATURE_HEAD": {"LINEAR_ENABLED": True, "LINEAR_OUT_FEATURES": 1024},
                        "LSTR": {"NUM_HEADS": 4, "DIM_FEEDFORWARD": 1024, "ACTIVATION": "relu", "LONG_MEMORY_NUM_SAMPLES": 64,
                                 "WORK_MEMORY_NUM_SAMPLES": 32, "ENC_MODULE": [[16, 1, True], [32, 2, True]], "DEC_MODULE": [-1, 2, True]}}}
    t = sa.OADConfig.from_reference_dict(thumos)
    assert (t.VISUAL_SIZE, t.d_model, t.NUM_HEADS, t.ENC_MODULE[0][0]) == (768, 1024, 4, 16) and t == sa.OADConfig()
    for bad in (dict(ACTIVATION="tanh"), dict(LONG_MEMORY_NUM_SAMPLES=0), dict(ENC_MODULE=[]), dict(ENC_MODULE=[[-1, 1, True]]),
                dict(NUM_HEADS=3), dict(MODALITY="audio"), dict(DEC_MODULE=[-1, 0, True])):
        with pytest.raises(ValueError):
            _config(c, **bad)
    with pytest.raises(ValueError, match="multiples of 64"):      # the library's width rule, before any weight exists
        sa.OnlineActionDetector(_config(c, VISUAL_SIZE=100))


@pytest.mark.parametrize("name", list(OO.CASES))
def test_state_dict_keys_are_the_reference_s(gold, name):
    import streamformer_amd as sa
    det = sa.OnlineActionDetector(_config(OO.CASES[name]))
    assert sorted(det.state_dict().keys()) == sorted(OO.state_dict_keys(gold, name))
    sd, _ = OO.golden_case(gold, name)
    res = det.load_state_dict(sd, strict=False)
    assert res.missing_keys == ["pos_encoding.pe"] and not res.unexpected_keys
    assert torch.equal(det.pos_encoding.pe[:20, 0], OO.positional_table(20, OO.CASES[name]["d_model"]))
    assert torch.equal(det.classifier.weight, sd["classifier.weight"])


def test_generation_tensors_are_ignored_and_listed(gold):
    import streamformer_amd as sa
    det = sa.OnlineActionDetector(_config(OO.CASES["a"]))
    sd = dict(det.state_dict())
    extra = {"gen_query.weight": torch.zeros(4, 128), "final_query.weight": torch.zeros(8, 128),
             "work_fusions.0.layers.0.linear1.weight": torch.zeros(192, 128), "gen_layer.norm.bias": torch.zeros(128)}
    res = det.load_state_dict({"model_state_dict": {**sd, **extra}})      # strict: the extra tensors are not "unexpected"
    assert not res.missing_keys and not res.unexpected_keys
    assert det.ignored_keys == sorted(extra)
    with pytest.raises(RuntimeError):
        det.load_state_dict({**sd, "classifier_verb.weight": torch.zeros(98, 128)})


def test_refusals():
    import streamformer_amd as sa
    c = OO.CASES["a"]
    with pytest.raises(NotImplementedError, match="MODALITY"):
        _config(c, MODALITY="twostream")
    with pytest.raises(NotImplementedError, match="EK100"):
        _config(c, DATA_NAME="EK100")
    with pytest.raises(ValueError, match="ENC_MODULE"):
        _config(c, ENC_MODULE=[[4, 2, True], [-1, 1, True]])
    fut = sa.OnlineActionDetector(_config(c, FUTURE_SECONDS=2))
    work = torch.zeros(1, c["work_samples"], c["d_in"])
    with pytest.raises(NotImplementedError, match="FUTURE_SECONDS"):
        fut.step(work, state=None)
    with pytest.raises(NotImplementedError, match="FUTURE_SECONDS"):
        fut(work, work)
    det = sa.OnlineActionDetector(_config(c))
    with pytest.raises(NotImplementedError, match="knn"):
        det(work, work)
    with pytest.raises(ValueError, match="every key"):
        det.step(work, [torch.zeros(c["long_samples"], c["d_in"])], torch.full((c["long_samples"],), NINF), state=None)
    with pytest.raises(ValueError, match="NaN"):
        det.step(work, None, torch.full((1, c["long_samples"]), float("nan")), state=None)
    with pytest.raises(ValueError, match="state"):
        det.step(work, None, None, state=None)
