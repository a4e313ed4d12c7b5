"""CPU: the ``trainable`` opt-in of the pixel decoder (what needs no GPU), and what the GPU gradient tests
(tests/test_pixel_decoder_train.py) lean on: the oracle's autograd gradients are right (central finite differences in fp64), the
GroupNorm backward formulas the kernels implement are right (numpy against torch fp64 autograd of ``F.group_norm``, with ReLU and with the
upsample), and no ReLU and no bilinear sample of the oracle is undecided at fp32 precision at the seeds the tests use (the cap is 0).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_decoder_oracle as PO
from tests import pixel_decoder_train_support as TS

EPS64 = 2.0 ** -53


def _module(c, **kw):
    import streamformer_amd as sa
    shape = {k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, c["channels"], PO.STRIDES)}
    return sa.MSDeformAttnPixelDecoder(shape, **dict(PO.decoder_kwargs(c), **kw))


# ------------------------------------------------------------------------------------------------
# the opt-in
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PO.CASES))
def test_trainable_keeps_the_parameter_tree(name):
    c = PO.CASES[name]
    a, b = _module(c), _module(c, trainable=True)
    assert not a.trainable and b.trainable
    assert list(a.state_dict()) == list(b.state_dict())
    assert [v.shape for v in a.state_dict().values()] == [v.shape for v in b.state_dict().values()]
    assert not b.load_state_dict(PO.make_weights(c), strict=True).missing_keys


def test_trainable_refusals_name_the_argument():
    c = PO.CASES["m2f"]
    with pytest.raises(ValueError, match="compute_dtype"):
        _module(c, trainable=True, compute_dtype="bf16")
    m = _module(c, compute_dtype="bf16")
    with pytest.raises(ValueError, match="compute_dtype"):
        m.trainable = True
    assert not m.trainable
    feats = PO.make_features(c)
    with pytest.raises(NotImplementedError, match="transformer_dropout"):
        _module(c, trainable=True, transformer_dropout=0.1).train().forward_features(feats)
    # dropout is never applied in eval: that path is the refusal of a CPU tensor, as without the opt-in
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _module(c, trainable=True, transformer_dropout=0.1).eval().forward_features(feats)


def test_forward_refusals_without_a_gpu():
    c = PO.CASES["m2f"]
    feats = PO.make_features(c)
    with pytest.raises(RuntimeError, match="inference only"):
        _module(c).train().forward_features(feats)
    with pytest.raises(RuntimeError, match="inference only"):
        _module(c, trainable=False).train()(feats)
    m = _module(c, trainable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train().forward_features(feats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval().forward_features(feats)
    m.trainable = False                      # the attribute takes the opt-in back
    with pytest.raises(RuntimeError, match="inference only"):
        m.train().forward_features(feats)


# ------------------------------------------------------------------------------------------------
# the oracle is fit for gradients
# ------------------------------------------------------------------------------------------------
FD_STEP = 1e-5
FD_TENSORS = ("layer_2.norm.weight", "adapter_3.weight", "layer_1.weight", "transformer.level_embed",
              "transformer.encoder.layers.0.self_attn.sampling_offsets.weight", "input_proj.0.1.bias", "mask_features.weight", "x.res5", "x.res2")


def test_oracle_gradients_against_finite_differences():
    """L = sum over the four outputs of <output, a fixed random cotangent>, in fp64, on ``res5only`` (one transformer level, three chained
    FPN levels: every operator of the decoder).  L is smooth up to ReLU kinks and bilinear corner changes, none of which is within reach
    of the step (test_no_relu_and_no_sample_is_undecided).  Along one random unit direction d per tensor, the central difference
    D(h) = (L(t + h d) - L(t - h d)) / 2 h with h = FD_STEP = 1e-5 must agree with <autograd gradient, d> within
        |D(2 h) - D(h)|          three times D(h)'s truncation error, which falls as h^2
      + 16 EPS64 A / h           the rounding of the two values of L it subtracts: L is a sum of terms of both signs whose absolute
                                 values add up to A, and each value carries a few (taken as 8) roundings of A."""
    name = "res5only"
    c = PO.CASES[name]
    run = TS.Run(name, torch.float64)
    cots = TS.cotangents(name, run.mask, run.out)
    grads = run.backward(cots)
    A = float(sum((t.detach() * ct).abs().sum() for t, ct in zip([run.mask] + run.out[:3], cots)))
    rs = np.random.RandomState(c["seed"] + 31)
    sd = {k: v.detach() for k, v in run.sd.items()}
    feats = {k: v.detach() for k, v in run.feats.items()}

    def loss(sd_, feats_):
        with torch.no_grad():
            mask, out = PO.forward(sd_, c, feats_, table="fp64")
            return float(TS.pairing(mask, out, cots, torch.float64))

    for key in FD_TENSORS:
        leaf = feats[key[2:]] if key.startswith("x.") else sd[key]
        d = torch.from_numpy(rs.standard_normal(tuple(leaf.shape)))
        d /= d.norm()                        # a unit direction: h is the length of the step
        analytic = float((grads[key] * d).sum())

        def at(step):
            moved = leaf + step * d
            if key.startswith("x."):
                return loss(sd, dict(feats, **{key[2:]: moved}))
            return loss(dict(sd, **{key: moved}), feats)

        D = lambda h: (at(h) - at(-h)) / (2 * h)      # noqa: E731
        d1, d2 = D(FD_STEP), D(2 * FD_STEP)
        bound = abs(d2 - d1) + 16 * EPS64 * A / FD_STEP
        print(f"  {name} {key}: autograd {analytic:.9e}, difference {d1:.9e}, gap {abs(d1 - analytic):.2e}, bound {bound:.2e}")
        assert abs(d1 - analytic) <= bound, (name, key, analytic, d1, bound)
        assert bound <= 1e-3 * max(abs(analytic), 1.0), (name, key, "the difference quotient decides nothing", bound, analytic)


@pytest.mark.parametrize("name", list(PO.CASES))
def test_no_relu_and_no_sample_is_undecided(name):
    """The cap on undecided pre-activations is 0: every pre-ReLU value of the fp64 oracle (GroupNorm's ReLU, the FFN's ReLU) lies further
    from zero than MARGIN x the fp32 floor of its tensor, and the fp32 oracle's sign pattern equals the fp64 one.  The same for the
    bilinear samples: every pixel coordinate lies further from an integer than MARGIN x the fp32 floor of the coordinates, and both runs
    sample the same corners."""
    close, flips, near, moved = TS.undecided(name)
    print(f"  {name} seed {TS.seed_of(name)}: pre-ReLU values inside the band {close}, sign flips {flips}; coordinates inside the band {near}, moved {moved}")
    assert (close, flips, near, moved) == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------
# the formulas of csrc/sf_pixdec_bwd.hip, in numpy
# ------------------------------------------------------------------------------------------------
def groupnorm_backward(x, gamma, beta, relu, dy, eps=PO.GN_EPS, groups=32):
    """rows x, dy [F, HW, C] -> (dx, dgamma, dbeta) by the kernels' formulas: per (frame, channel) b = sum g, a = sum g xhat; per
    (frame, group) s1 = sum_c gamma_c b, s2 = sum_c gamma_c a; dx = rstd (g gamma - s1 / n - xhat s2 / n)."""
    Fr, HW, C = x.shape
    cg = C // groups
    xg = x.reshape(Fr, HW, groups, cg)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(xg.var(axis=(1, 3), keepdims=True) + eps)
    xhat = ((xg - mean) * rstd).reshape(Fr, HW, C)
    g = np.where(xhat * gamma + beta <= 0, 0.0, dy) if relu else dy
    b, a = g.sum(axis=1), (g * xhat).sum(axis=1)                                  # [F, C]
    n = HW * cg
    s1 = (gamma * b).reshape(Fr, groups, cg).sum(-1) / n                          # [F, G]
    s2 = (gamma * a).reshape(Fr, groups, cg).sum(-1) / n
    rep = lambda t: np.repeat(t, cg, axis=-1)[:, None, :]                         # noqa: E731
    dx = rep(rstd.reshape(Fr, groups)) * (g * gamma - rep(s1) - xhat * rep(s2))
    return dx, a.sum(0), b.sum(0)


def bilinear_axis(dst, ratio, n_in):
    """sf_bilinear_axis (csrc/sf_nchw_tile.h) in fp64."""
    src = max(ratio * (dst + 0.5) - 0.5, 0.0)
    a = min(int(src), n_in - 1)
    return a, min(a + 1, n_in - 1), min(src - a, 1.0)


def upsample_backward(dy, H, W, Hp, Wp):
    """rows dy [F, H W, C] -> d_prev [F, Hp Wp, C] in the kernel's gather form: a coarse pixel adds the fine pixels whose taps land on it."""
    Fr, _, C = dy.shape
    out = np.zeros((Fr, Hp, Wp, C))
    dy = dy.reshape(Fr, H, W, C)
    wy = np.zeros((H, Hp))
    wx = np.zeros((W, Wp))
    for w, n, n_in in ((wy, H, Hp), (wx, W, Wp)):
        for i in range(n):
            i0, i1, l1 = bilinear_axis(i, n_in / n, n_in)
            w[i, i0] += 1.0 - l1
            w[i, i1] += l1
    for yp in range(Hp):
        for xp in range(Wp):
            for y in np.nonzero(wy[:, yp])[0]:
                for x in np.nonzero(wx[:, xp])[0]:
                    out[:, yp, xp] += wy[y, yp] * wx[x, xp] * dy[:, y, x]
    return out.reshape(Fr, Hp * Wp, C)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C_,H,W", [(64, 1, 1), (64, 3, 5), (128, 7, 9), (256, 2, 3)])
def test_groupnorm_backward_formulas(C_, H, W, relu):
    rs = np.random.RandomState(2800 + C_ + 7 * H + W)
    x = rs.standard_normal((2, H * W, C_))
    gamma, beta, dy = 1.0 + 0.1 * rs.standard_normal(C_), 0.1 * rs.standard_normal(C_), rs.standard_normal((2, H * W, C_))
    xt, gt, bt = (torch.from_numpy(t).requires_grad_() for t in (x, gamma, beta))
    y = F.group_norm(PO.to_map(xt, H, W), 32, gt, bt, PO.GN_EPS)
    (PO.to_rows(torch.relu(y) if relu else y) * torch.from_numpy(dy)).sum().backward()
    dx, dgamma, dbeta = groupnorm_backward(x, gamma, beta, relu, dy)
    # two fp64 evaluations of one formula: they differ by roundings of the terms dx is the difference of.  With one pixel and two
    # channels per group rstd reaches 1 / sqrt(eps) = 316 and those terms are rstd^2 = 1e5 times a result of order 1: 1e5 * 2^-53 = 1e-11,
    # a few of them 1e-10
    for got, want in ((dx, xt.grad), (dgamma, gt.grad), (dbeta, bt.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-10 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("src,dst", [((2, 3), (3, 5)), ((4, 4), (7, 7)), ((1, 1), (4, 4)), ((7, 7), (13, 15)), ((5, 4), (2, 3))])
def test_upsample_backward_formula(src, dst):
    rs = np.random.RandomState(2820 + 11 * dst[0] + dst[1])
    C_ = 8
    dy = rs.standard_normal((2, dst[0] * dst[1], C_))
    prev = torch.from_numpy(rs.standard_normal((2, C_, *src))).requires_grad_()
    up = F.interpolate(prev, size=dst, mode="bilinear", align_corners=False)
    (PO.to_rows(up) * torch.from_numpy(dy)).sum().backward()
    got = upsample_backward(dy, *dst, *src)
    assert np.abs(got - PO.to_rows(prev.grad).numpy()).max() <= 1e-12
