"""CPU: the training restatement of the ViT-Adapter (tests/vit_adapter_train_support.py) against fixture F27 (the reference's own class in
``.train()``, fp64, tools/make_golden_vit_adapter_train.py), the ReLU and max-pool check of its inputs, and what the module refuses.

F27 against the restatement: names, shapes and integer content are equal, floats agree to 1e-10 of the array's largest magnitude.  Two
gradients are ZERO in exact arithmetic, ``up.bias`` and ``spm.fc1.bias``: both are added in front of a BatchNorm that subtracts the batch
mean, so what either side holds is the rounding residue of a cancelling sum (about 1e-13 against a weight gradient of 1e2).  Their scale
is that of the same layer's weight gradient, whose summands they share.
"""
import numpy as np
import pytest
import torch

from tests import vit_adapter_oracle as VO
from tests import vit_adapter_train_support as TS
from tests.helpers import NoLaunch

ZERO_BY_BATCHNORM = {"up.bias": "up.weight", "spm.fc1.bias": "spm.fc1.weight"}


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in VO.CASES:
        r = TS.Run(name, torch.float64)
        out[name] = (r, r.backward(TS.cotangents(name, r.outs)))
    return out


@pytest.mark.parametrize("name", list(VO.CASES))
def test_restatement_reproduces_f27(name, runs):
    r, grads = runs[name]
    got, want = TS.golden_arrays(name, dict(outs=r.outs, stats=r.stats), grads), TS.load_golden(name)
    assert sorted(got) == sorted(want)
    assert list(want["grad_keys"]) == sorted(TS.trainable_keys(r.sd))
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if w.dtype.kind != "f":
            assert np.array_equal(g, w), k
            continue
        scale = np.abs(w).max()
        if k[len("grad."):] in ZERO_BY_BATCHNORM:
            scale = max(scale, want["grad." + ZERO_BY_BATCHNORM[k[len("grad."):]]][0])      # the weight gradient's max-abs
        rel = np.abs(g - w).max() / scale
        worst = max(worst, rel)
        assert rel <= 1e-10, (k, rel)
    print(f"  {name}: {len(want)} arrays, largest relative difference {worst:.2e}")
    assert all(v.size * v.itemsize <= 1 << 20 for v in want.values())


@pytest.mark.parametrize("name", list(VO.CASES))
def test_no_relu_and_no_pool_window_is_undecided(name):
    """Cap 0: no pre-ReLU value of the fp64 oracle inside MARGIN x the fp32 floor of its tensor, no max-pool window whose top-two margin is,
    and fp32 and fp64 clip and pick identically."""
    assert TS.undecided(name) == (0, 0, 0, 0)


def test_running_statistics_move_by_the_momentum_rule(runs):
    r, _ = runs["sq"]
    before = TS.weights("sq")
    for k, v in r.stats.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1
        else:
            assert not torch.allclose(v, before[k].double())
    assert len(r.stats) == 3 * (6 + 4)


def _adapter(c, **kw):
    import streamformer_amd as sa
    return sa.TimesformerMultiTaskingModelSigLIPViTAdapter(kw.pop("config", VO.config(c)), **dict(VO.adapter_kwargs(c), **kw))


def test_opt_in_and_refusals(monkeypatch):
    import streamformer_amd.adapter as A
    c = VO.CASES["sq"]
    with pytest.raises(ValueError, match="trainable=True needs compute_dtype='fp32'"):
        _adapter(c, compute_dtype="bf16", trainable=True)
    m = _adapter(c, compute_dtype="bf16")
    with pytest.raises(ValueError, match="trainable=True"):
        m.trainable = True
    assert _adapter(c).trainable is False and _adapter(c, trainable=True).trainable is True
    with pytest.raises(NotImplementedError, match="with_cp"):
        _adapter(c, with_cp=True, trainable=True)
    # every .train() refusal comes before anything is launched, on any device
    probe = NoLaunch(A.nat)
    monkeypatch.setattr(A, "nat", probe)
    px = torch.zeros(1, 2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="inference only.*trainable=True"):
        _adapter(c).train()(px)
    with pytest.raises(NotImplementedError, match="freeze_backbone=False"):
        _adapter(c, trainable=True, freeze_backbone=False).train()(px)
    m = _adapter(c, trainable=True)
    m.encoder.layer[1].output.dense.bias.requires_grad = True
    with pytest.raises(NotImplementedError, match=r"encoder\.layer\.1\.output\.dense\.bias requires a gradient"):
        m.train()(px)
    base = VO.config(c).to_dict()
    base.pop("model_type", None)
    import streamformer_amd as sa
    for field in ("hidden_dropout_prob", "attention_probs_dropout_prob", "drop_path_rate"):
        m = _adapter(c, config=sa.StreamformerConfig(**dict(base, **{field: 0.1})), trainable=True)
        with pytest.raises(NotImplementedError, match=field):
            m.train()(px)
    m = _adapter(c, trainable=True).train()
    with pytest.raises(RuntimeError, match="runs on the MI355X"):      # accepted up to the device check
        m(px)
    assert probe.calls == []
