"""CPU: the ``trainable`` opt-in of the two mask decoder classes (what needs no GPU), and the two properties of the oracle that the
GPU gradient tests (tests/test_mask_decoder_train.py) lean on: its autograd gradients are right (central finite differences in fp64),
and its own attention masks are decidable at fp32 precision (the share of bits inside the band stays under the cap).
"""
import functools

import numpy as np
import pytest
import torch

from tests import mask_decoder_oracle as DO
from tests.helpers import EPS32, MARGIN, maxabs

CAP = 0.05
EPS64 = 2.0 ** -53


def _module(c, **kw):
    import streamformer_amd as sa
    return getattr(sa, c["cls"])(c["in_channels"], **dict(DO.decoder_kwargs(c), **kw))


@pytest.mark.parametrize("name", list(DO.CASES))
def test_trainable_keeps_the_parameter_tree(name):
    c = DO.CASES[name]
    a, b = _module(c), _module(c, trainable=True)
    assert not a.trainable and b.trainable
    assert list(a.state_dict()) == list(b.state_dict())
    assert [v.shape for v in a.state_dict().values()] == [v.shape for v in b.state_dict().values()]
    assert not b.load_state_dict(DO.make_weights(c), strict=True).missing_keys


def test_trainable_refusals_name_the_argument():
    c = DO.CASES["cl"]
    for cls_case in (c, DO.CASES["m2f"]):
        with pytest.raises(ValueError, match="compute_dtype"):
            _module(cls_case, trainable=True, compute_dtype="bf16")
    m = _module(c, compute_dtype="bf16")
    with pytest.raises(ValueError, match="compute_dtype"):
        m.trainable = True
    assert not m.trainable
    with pytest.raises(NotImplementedError, match="pre_norm"):
        _module(c, trainable=True, pre_norm=True)
    with pytest.raises(NotImplementedError, match="mask_classification"):
        _module(c, trainable=True, mask_classification=False)


def test_forward_refusals_without_a_gpu():
    c = DO.CASES["cl"]
    xs, mf = DO.make_inputs(c)
    with pytest.raises(RuntimeError, match="inference only"):
        _module(c, trainable=False).train()(xs, mf)
    m = _module(c, trainable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train()(xs, mf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(xs, mf)
    m.trainable = False                      # the attribute takes the opt-in back
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(xs, mf)


# ------------------------------------------------------------------------------------------------
# the oracle is fit for gradients
# ------------------------------------------------------------------------------------------------
PRED_KEYS = ("pred_logits", "pred_masks", "pred_queries", "pred_embeds")
FD_STEP = 1e-5
FD_TENSORS = ("transformer_cross_attention_layers.0.multihead_attn.in_proj_weight", "decoder_norm.weight", "query_embed.weight", "mask_features")


@functools.lru_cache(maxsize=None)
def _free(name):
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c)
    with torch.no_grad():
        return DO.forward(DO.make_weights(c), c, xs, mf, table="fp64")


@pytest.mark.parametrize("name", list(DO.CASES))
def test_oracle_gradients_against_finite_differences(name):
    """L = sum over every differentiable output (final and aux) of <output, a fixed random cotangent>, in fp64, attention masks forced to
    the oracle's own thresholds (L is then smooth up to ReLU kinks).  Along one random unit direction d per tensor, the central difference
    D(h) = (L(t + h d) - L(t - h d)) / 2 h with h = FD_STEP = 1e-5 must agree with <autograd gradient, d> within
        |D(2 h) - D(h)|          three times D(h)'s truncation error, which falls as h^2
      + 16 EPS64 A / h           the rounding of the two values of L it subtracts: L is a sum of terms of both signs whose absolute
                                 values add up to A, and each value carries a few (taken as 8) roundings of A."""
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c)
    masks = _free(name)["attn_masks"]
    rs = np.random.RandomState(c["seed"] + 31)
    free = _free(name)
    cots = [{k: torch.from_numpy(rs.standard_normal(tuple(p[k].shape))) for k in PRED_KEYS if k in p} for p in free["aux"] + [free]]

    def loss(sd, mfeat, absolute=False):
        res = DO.forward(sd, c, xs, mfeat, table="fp64", masks=masks)
        return sum(((p[k] * v).abs() if absolute else p[k] * v).sum() for p, ct in zip(res["aux"] + [res], cots) for k, v in ct.items())

    sd = {k: v.double().requires_grad_() for k, v in DO.make_weights(c).items()}
    mf64 = mf.double().requires_grad_()
    loss(sd, mf64).backward()
    with torch.no_grad():
        A = float(loss(sd, mf64, absolute=True))
    for key in FD_TENSORS:
        leaf = mf64 if key == "mask_features" else sd[key]
        d = torch.from_numpy(rs.standard_normal(tuple(leaf.shape)))
        d /= d.norm()                        # a unit direction: h is the length of the step
        analytic = float((leaf.grad * d).sum())

        def at(step):
            with torch.no_grad():
                moved = leaf.detach() + step * d
                if key == "mask_features":
                    return float(loss({k: v.detach() for k, v in sd.items()}, moved))
                return float(loss({k: (moved if k == key else v.detach()) for k, v in sd.items()}, mf64.detach()))

        D = lambda h: (at(h) - at(-h)) / (2 * h)      # noqa: E731
        d1, d2 = D(FD_STEP), D(2 * FD_STEP)
        bound = abs(d2 - d1) + 16 * EPS64 * A / FD_STEP
        print(f"  {name} {key}: autograd {analytic:.9e}, difference {d1:.9e}, gap {abs(d1 - analytic):.2e}, bound {bound:.2e}")
        assert abs(d1 - analytic) <= bound, (name, key, analytic, d1, bound)
        assert bound <= 1e-3 * max(abs(analytic), 1.0), (name, key, "the difference quotient decides nothing", bound, analytic)


@pytest.mark.parametrize("name", list(DO.CASES))
def test_oracle_masks_are_decidable_in_fp32(name):
    """An fp32 run of the oracle attending under ITS OWN thresholds against the fp64 run: outside the band (MARGIN x the fp32 floor of the
    layer's low-resolution logits) every bit agrees, so the two runs attend alike, and the share of bits inside the band stays under CAP."""
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c)
    sd = DO.make_weights(c)
    want = _free(name)
    with torch.no_grad():
        floor = DO.forward(sd, c, xs, mf, dtype=torch.float32, operands=False, table="fp64", masks=want["attn_masks"])
        own = DO.forward(sd, c, xs, mf, dtype=torch.float32, operands=False, table="fp64")
    diverged = False
    for i, (w, f) in enumerate(zip(want["low_logits"], floor["low_logits"])):
        band = MARGIN * max(maxabs(f, w), EPS32 * float(w.abs().max()))
        inside = w.abs() <= band
        share = float(inside.double().mean())
        print(f"  {name} layer {i}: band {band:.3e}, share inside {share:.4f}")
        assert share < CAP, (name, i, share)
        raw32, raw64 = own["low_logits"][i] < 0, w < 0
        if not diverged:                     # until an undecided bit falls differently the two runs have attended alike
            assert torch.equal(raw32[~inside], raw64[~inside]), (name, i, "a decided bit differs between the fp32 and the fp64 run")
        diverged = diverged or not torch.equal(raw32, raw64)
