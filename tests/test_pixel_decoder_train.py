"""Training the native pixel decoder on the MI355X: the two backward entries alone against fp64 torch autograd at every shape at which
they take another path, and the ``trainable=True`` module in ``.train()`` against fp64 autograd of the restated reference
(tests/pixel_decoder_oracle.py, run by tests/pixel_decoder_train_support.py).

Tolerances are those of tests/test_pixel_decoder.py: MARGIN = 4 times the PRECISION FLOOR of what is bounded (the same torch operator
sequence in fp32 on the CPU against fp64, never less than one fp32 rounding of the result), computed here from the inputs and never
from the code under test.  Gradients are bounded per tensor, relative to that tensor's largest magnitude.  A ReLU whose pre-activation
is within rounding of zero flips its gradient discretely: the inputs of the entry tests are moved off zero until none is inside the
band, and tests/test_pixel_decoder_train_cpu.py shows the same (cap 0) for the oracle of the module tests.

The partial pass gives a workgroup 64 pixel rows at these sizes (PXD_BWD_MIN_SPAN_ROWS, csrc/sf_pixdec_bwd.hip): 12 x 20 = 240 rows are
four spans, the other grids one.

Bit-equality of two training steps is claimed for the outputs and for every gradient that does not pass through the float atomics of
``sf_op_msda_backward``'s grad_value: the FPN's 1 x 1 convolutions and GroupNorms (adapter_*, layer_*.norm), mask_features, the inputs of
the FPN levels, and the LAST encoder layer's output_proj, sampling_offsets, attention_weights, norms and linears.  Everything upstream of
a grad_value (value_proj, earlier layers, input_proj, level_embed, the transformer's input levels) is compared against the bound only, and
so is the 3 x 3 convolution's weight (layer_*.weight): its gradient is torch's ``F.conv2d`` backward, which on this GPU gave different
last bits in two runs.

Measured on an MI355X (largest error / bound): GroupNorm backward entry dx 0.36, dgamma 0.61, dbeta 0.58; upsample adjoint 0.25; module
outputs 0.34; gradients per group over the three cases: attention 0.58, ffn 0.42, norms 0.42, fpn 0.48, input_proj 0.46, level_embed 0.28,
mask_features 0.37, x 0.55.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_decoder_oracle as PO
from tests import pixel_decoder_train_support as TS
from tests.conftest import ROOT
from tests.helpers import EPS32, MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream, draw as _draw

pytestmark = pytest.mark.gpu

FR = TS.FRAMES
GRIDS = [(1, 1), (3, 5), (7, 9), (12, 20)]


def _ratio(got, floor32, want):
    return maxabs(got, want) / (MARGIN * fp32_floor(floor32, want))


def _rows(x):
    return x.flatten(2).transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------
# 1. GroupNorm backward alone
# ------------------------------------------------------------------------------------------------
def _gn_autograd(x, gamma, beta, relu, dy, dt):
    """x, dy NCHW -> (dx NCHW, dgamma, dbeta, pre-ReLU value) by torch autograd in ``dt``."""
    xt, gt, bt = (t.detach().clone().to(dt).requires_grad_() for t in (x, gamma, beta))
    pre = F.group_norm(xt, 32, gt, bt, PO.GN_EPS)
    ((torch.relu(pre) if relu else pre) * dy.to(dt)).sum().backward()
    return xt.grad, gt.grad, bt.grad, pre.detach()


def _off_zero(x, gamma, beta):
    """x with every element whose pre-ReLU value is inside the band (MARGIN x the fp32 floor of the pre-ReLU tensor) moved by 1/8 (exact
    in fp32 at these magnitudes) until none is left; asserts the cap of 0 and that fp32 and fp64 clip the same elements."""
    x = x.clone()
    for _ in range(8):
        pre64 = F.group_norm(x.double(), 32, gamma.double(), beta.double(), PO.GN_EPS)
        pre32 = F.group_norm(x, 32, gamma, beta, PO.GN_EPS)
        inside = pre64.abs() <= MARGIN * fp32_floor(pre32, pre64)
        if not inside.any():
            assert torch.equal(pre32 > 0, pre64 > 0)
            return x
        x[inside] += 0.125
    raise AssertionError("pre-ReLU values stay inside the band")


def _gn_forward(nat, dev, xd, gd, bd, relu, H, W):
    """The forward entry on rows xd: (stats, y rows on the device)."""
    Fr, _, C_ = xd.shape
    stats = torch.empty(Fr, 32, 4, device=dev)
    y = torch.empty_like(xd)
    nat.check(nat.lib.sf_op_pixdec_groupnorm(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), int(relu), None, 0, 0, None, stats.data_ptr(), y.data_ptr(), None, None,
                                             None, None, Fr, H, W, C_, _stream()))
    return stats, y


def _gn_backward(nat, dev, xd, stats, gd, bd, relu, dyd, H, W, want=(True, True, True)):
    """-> (dx rows, dgamma, dbeta) on the CPU after the guard checks; an output that is not asked for must stay unwritten."""
    Fr, _, C_ = xd.shape
    bufs = [guarded(dev, Fr, H * W, C_), guarded(dev, C_), guarded(dev, C_)]
    nbytes = nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(Fr, H, W, C_)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device=dev)
    ptrs = [v.data_ptr() if w else None for (_, v), w in zip(bufs, want)]
    nat.check(nat.lib.sf_op_pixdec_groupnorm_backward(xd.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), int(relu), dyd.data_ptr(), *ptrs,
                                                      Fr, H, W, C_, ws.data_ptr(), nbytes, _stream()))
    torch.cuda.synchronize()
    assert (ws[nbytes:].cpu() == 0x5a).all(), "the workspace's guard was written"
    out = []
    for (buf, view), w in zip(bufs, want):
        if w:
            out.append(read_guarded(buf, view))
        else:
            assert torch.isnan(buf.cpu()).all(), "an output was written although NULL was passed"
            out.append(None)
    return out


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("C_", [64, 128, 256])
def test_groupnorm_backward_entry(C_, H, W):
    nat, dev = _nat(), gpu_device()
    rs = np.random.RandomState(2900 + C_ + 7 * H + W)
    gamma, beta = 1.0 + 0.1 * _draw(rs, C_), 0.1 * _draw(rs, C_)
    base = _draw(rs, FR, C_, H, W)
    sign = 1.0 - 2.0 * (torch.arange(32) % 2)
    drawings = {"normal": base, "offset100": base + 100.0 * sign.repeat_interleave(C_ // 32)[None, :, None, None]}      # mean^2 / variance = 1e4
    dy = _draw(rs, FR, C_, H, W)
    gd, bd, dyd = gamma.to(dev), beta.to(dev), _rows(dy).to(dev)
    single = nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(FR, 1, 1, C_)
    many = nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(FR, H, W, C_)
    assert (many > single) == ((H, W) == (12, 20)), "12 x 20 must split into more than one span, the smaller grids must not"
    worst = dict(dx=0.0, dgamma=0.0, dbeta=0.0)
    for name, x in drawings.items():
        x = _off_zero(x, gamma, beta)
        xd = _rows(x).to(dev)
        for relu in (False, True):
            tag = (C_, H, W, name, relu)
            stats, _ = _gn_forward(nat, dev, xd, gd, bd, relu, H, W)
            got = _gn_backward(nat, dev, xd, stats, gd, bd, relu, dyd, H, W)
            want = _gn_autograd(x, gamma, beta, relu, dy, torch.float64)
            floor = _gn_autograd(x, gamma, beta, relu, dy, torch.float32)
            for key, g, f32, w in (("dx", got[0], _rows(floor[0]), _rows(want[0])), ("dgamma", got[1], floor[1], want[1]), ("dbeta", got[2], floor[2], want[2])):
                r = _ratio(g, f32, w)
                worst[key] = max(worst[key], r)
                assert r <= 1.0, (tag, key, r)
            again = _gn_backward(nat, dev, xd, stats, gd, bd, relu, dyd, H, W)
            assert all(torch.equal(a, b) for a, b in zip(again, got)), (tag, "a second run differs")
            for i, key in enumerate(("dx", "dgamma", "dbeta")):
                alone = _gn_backward(nat, dev, xd, stats, gd, bd, relu, dyd, H, W, want=tuple(j == i for j in range(3)))
                assert torch.equal(alone[i], got[i]), (tag, key, "alone differs from the joint run")
    print(f"  groupnorm backward C={C_} {H}x{W}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("C_", [64, 256])
def test_groupnorm_backward_clips_exactly_where_the_forward_clipped(C_):
    """dy = 1 everywhere: dbeta[c] counts the elements of channel c that the backward lets through, an integer that fp32 holds exactly.
    It must equal the count of positive outputs of the forward kernel, also where a pre-ReLU value is within rounding of zero: the
    inputs here are NOT moved off zero, and beta = 0 with a third of the pixels at their group's mean puts values on the edge."""
    nat, dev = _nat(), gpu_device()
    H, W = 12, 20
    rs = np.random.RandomState(2950 + C_)
    x = _rows(_draw(rs, FR, C_, H, W))
    kept = torch.arange(H * W) % 3 != 0                          # every third pixel is set to the mean of the others: it stays the group's mean
    mean = x[:, kept].double().view(FR, -1, 32, C_ // 32).mean(dim=(1, 3), keepdim=True).expand(-1, H * W, -1, C_ // 32).reshape(FR, H * W, C_)
    x[:, ~kept] = mean[:, ~kept].float()
    gamma, beta = 1.0 + 0.1 * _draw(rs, C_), torch.zeros(C_)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    stats, y = _gn_forward(nat, dev, xd, gd, bd, True, H, W)
    ones = torch.ones_like(xd)
    _, _, dbeta = _gn_backward(nat, dev, xd, stats, gd, bd, True, ones, H, W, want=(False, False, True))
    passed = (y > 0).sum(dim=(0, 1)).cpu()
    assert 0 < int(passed.sum()) < y.numel()
    assert torch.equal(dbeta, passed.float())


# ------------------------------------------------------------------------------------------------
# 2. the upsample's adjoint alone
# ------------------------------------------------------------------------------------------------
def _up_autograd(dy, src, dst, dt):
    prev = torch.zeros(dy.shape[0], dy.shape[1], *src, dtype=dt, requires_grad=True)
    (F.interpolate(prev, size=dst, mode="bilinear", align_corners=False) * dy.to(dt)).sum().backward()
    return _rows(prev.grad)


@pytest.mark.parametrize("src,dst", [((2, 3), (3, 5)), ((4, 4), (7, 7)), ((1, 1), (4, 4)), ((7, 7), (13, 15))])
@pytest.mark.parametrize("C_", [64, 128])
def test_upsample_backward_entry(C_, src, dst):
    nat, dev = _nat(), gpu_device()
    dy = _draw(np.random.RandomState(2960 + C_ + 11 * dst[0] + dst[1]), FR, C_, *dst)
    dy[1] += 1000.0                           # a fine pixel taken from the other frame shows at once
    dyd = _rows(dy).to(dev)

    def run():
        buf, out = guarded(dev, FR, src[0] * src[1], C_)
        nat.check(nat.lib.sf_op_pixdec_upsample_backward(dyd.data_ptr(), out.data_ptr(), FR, dst[0], dst[1], src[0], src[1], C_, _stream()))
        torch.cuda.synchronize()
        return read_guarded(buf, out)

    got = run()
    check_against_floor(f"upsample adjoint {dst} -> {src} C={C_}", got, _up_autograd(dy, src, dst, torch.float32), _up_autograd(dy, src, dst, torch.float64))
    assert torch.equal(run(), got), "a second run differs"


# ------------------------------------------------------------------------------------------------
# 3. refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refusals():
    nat, dev = _nat(), gpu_device()
    t = torch.zeros(1 << 16, device=dev)
    p = t.data_ptr()
    K = 1 << 10

    def gn(x=p, stats=p, gamma=p, beta=p, dy=p, dx=p + 64 * K, dg=p + 128 * K, db=p + 129 * K, ws=p + 192 * K, ws_bytes=32 * K, F_=2, H=2, W=2, C_=64):
        return nat.lib.sf_op_pixdec_groupnorm_backward(x, stats, gamma, beta, 1, dy, dx, dg, db, F_, H, W, C_, ws, ws_bytes, _stream())

    def up(dy=p, d_prev=p + 64 * K, F_=2, H=3, W=5, Hp=2, Wp=3, C_=64):
        return nat.lib.sf_op_pixdec_upsample_backward(dy, d_prev, F_, H, W, Hp, Wp, C_, _stream())

    assert gn() == nat.SF_OK and up() == nat.SF_OK
    shapes = (dict(C_=0), dict(C_=96), dict(C_=-64), dict(F_=0), dict(F_=65536), dict(H=0), dict(W=0))
    for kw in (dict(x=None), dict(stats=None), dict(gamma=None), dict(beta=None), dict(dy=None), dict(ws=None), dict(dx=None, dg=None, db=None), dict(x=p + 4),
               dict(stats=p + 8), dict(gamma=p + 4), dict(beta=p + 4), dict(dy=p + 12), dict(dx=p + 64 * K + 4), dict(dg=p + 128 * K + 4),
               dict(db=p + 129 * K + 8), dict(ws=p + 192 * K + 16)) + shapes:
        assert gn(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_pixdec_groupnorm_backward" in nat.lib.sf_last_error()
    assert gn(ws_bytes=256) == nat.SF_ERR_WORKSPACE and b"workspace" in nat.lib.sf_last_error()
    assert gn(F_=65535, H=256, W=256) == nat.SF_ERR_CAPACITY
    assert nat.lib.sf_op_pixdec_groupnorm_backward_workspace_bytes(65535, 256, 256, 64) == 0
    for kw in (dict(dy=None), dict(d_prev=None), dict(dy=p + 4), dict(d_prev=p + 64 * K + 8), dict(Hp=0), dict(Wp=0)) + shapes:
        assert up(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_pixdec_upsample_backward" in nat.lib.sf_last_error()
    assert up(F_=65535, H=256, W=256) == nat.SF_ERR_CAPACITY and up(F_=65535, Hp=256, Wp=256) == nat.SF_ERR_CAPACITY
    torch.cuda.synchronize()
    assert not t.any()                                         # zeros in: the accepted calls wrote zeros, the refused ones nothing


# ------------------------------------------------------------------------------------------------
# 4. the module
# ------------------------------------------------------------------------------------------------
def _module(name, trainable=True, **kw):
    import streamformer_amd as sa
    c = PO.CASES[name]
    shape = {k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, c["channels"], PO.STRIDES)}
    m = sa.MSDeformAttnPixelDecoder(shape, **dict(PO.decoder_kwargs(c), **kw), trainable=trainable)
    m.load_state_dict(TS.weights(name), strict=True)
    return m.to(gpu_device())


def _group(name):
    if name.startswith("x."):
        return "x"
    for g, label in (("self_attn", "attention"), ("linear", "ffn"), ("norm1", "norms"), ("norm2", "norms"), ("level_embed", "level_embed"),
                     ("input_proj", "input_proj"), ("adapter_", "fpn"), ("layer_", "fpn"), ("mask_features", "mask_features")):
        if g in name:
            return label
    raise AssertionError(name)


def _past_the_atomics(name, c):
    """Whether the gradient ``name`` is computed without passing through sf_op_msda_backward's grad_value (the file's docstring)."""
    last = f"transformer.encoder.layers.{c['layers'] - 1}."
    if name.startswith("layer_") and name.endswith(".weight") and "norm" not in name:
        return False                          # torch's convolution weight gradient: not bit-reproducible on this GPU
    if name.startswith(("adapter_", "layer_", "mask_features")):
        return True
    if name.startswith("x."):
        return PO.LEVELS.index(name[2:]) < PO.num_fpn(c)
    return name.startswith(last) and "value_proj" not in name


def _step(m, name, cots):
    dev = gpu_device()
    m.zero_grad(set_to_none=True)
    feats = {k: v.to(dev).requires_grad_() for k, v in TS.features(name).items()}
    mask, first, ms = m.forward_features(feats)
    assert first is ms[0] and len(ms) == 3
    TS.pairing(mask, ms, cots, torch.float32).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({f"x.{k}": v.grad for k, v in feats.items()})
    return mask.detach(), [t.detach() for t in ms], grads


@pytest.mark.parametrize("name", list(PO.CASES))
def test_module_gradients(name):
    c = PO.CASES[name]
    want, floor = TS.Run(name, torch.float64), TS.Run(name, torch.float32)
    cots = TS.cotangents(name, want.mask, want.out)
    want_g, floor_g = want.backward(cots), floor.backward(cots)
    m = _module(name).train()
    mask, ms, grads = _step(m, name, cots)
    assert mask.shape == want.mask.shape and [t.shape for t in ms] == [t.shape for t in want.out[:3]]
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in [mask] + ms)
    check_against_floor(f"{name} train mask_features", mask, floor.mask.detach(), want.mask.detach())
    for i, t in enumerate(ms):
        check_against_floor(f"{name} train out[{i}]", t, floor.out[i].detach(), want.out[i].detach())
    assert sorted(grads) == sorted(want_g)
    worst = {}
    for k, w in want_g.items():
        assert w is not None and grads[k] is not None, (k, "has no gradient")
        assert grads[k].shape == w.shape, k
        g = _group(k)
        worst[g] = max(worst.get(g, 0.0), _ratio(grads[k], floor_g[k], w))
    print(f"  {name} gradients, largest error / bound per group: " + ", ".join(f"{g} {r:.3f}" for g, r in sorted(worst.items())))
    for k, w in want_g.items():
        check_against_floor(f"{name} grad {k}", grads[k], floor_g[k], w)
    # a second forward + backward: the same bits where no float atomic is passed
    mask2, ms2, grads2 = _step(m, name, cots)
    assert torch.equal(mask2, mask) and all(torch.equal(a, b) for a, b in zip(ms2, ms))
    fixed = [k for k in grads if _past_the_atomics(k, c)]
    assert len(fixed) >= 10
    moved = [k for k in fixed if not torch.equal(grads2[k], grads[k])]
    print(f"  {name}: {len(fixed)} gradients claimed bit-equal; of the others, equal in this run: "
          f"{sum(torch.equal(grads2[k], grads[k]) for k in grads if k not in fixed)} of {len(grads) - len(fixed)}")
    assert not moved, (moved, "differ between two runs")


@pytest.mark.parametrize("name", list(PO.CASES))
def test_eval_path_is_untouched(name):
    dev = gpu_device()
    feats = {k: v.to(dev) for k, v in TS.features(name).items()}
    plain, tr = _module(name, trainable=False).eval(), _module(name).eval()
    a, b = plain.forward_features(feats), tr.forward_features(feats)
    assert torch.equal(a[0], b[0]) and len(a[2]) == len(b[2]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert not any(t.requires_grad for t in [b[0]] + b[2])
    with pytest.raises(RuntimeError, match="inference only"):
        plain.train().forward_features(feats)
    tr.trainable = False
    with pytest.raises(RuntimeError, match="inference only"):
        tr.train().forward_features(feats)


# ------------------------------------------------------------------------------------------------
# 5. pixel decoder -> mask decoder -> criterion -> backward
# ------------------------------------------------------------------------------------------------
def test_chain_with_the_mask_decoder_and_the_criterion():
    import streamformer_amd as sa
    name, dev = "m2f", gpu_device()
    c = PO.CASES[name]
    classes = 5
    pix = _module(name).train()
    torch.manual_seed(2990)
    dec = sa.MultiScaleMaskedTransformerDecoder(c["conv_dim"], num_classes=classes, hidden_dim=64, num_queries=8, nheads=4, dim_feedforward=128, dec_layers=3,
                                                pre_norm=False, mask_dim=c["mask_dim"], enforce_input_project=True, trainable=True).to(dev).train()
    H, W = c["grids"][0]
    targets = []
    for f in range(FR):                                        # two planted targets per frame: the left and the right half
        masks = torch.zeros(2, 2 * H, 2 * W)
        masks[0, :, :W], masks[1, :, W:] = 1.0, 1.0
        targets.append({"labels": torch.tensor([f % classes, (f + 1) % classes], device=dev), "masks": masks.to(dev)})
    g = torch.Generator(device="cpu").manual_seed(5)
    rand = lambda shape, device: torch.rand(*shape, generator=g).to(device)      # noqa: E731
    crit = sa.SetCriterion(classes, sa.HungarianMatcher(2.0, 5.0, 5.0, num_points=32, rand=rand), {}, 0.1, ["labels", "masks"], 32, 3.0, 0.75,
                           rand=rand).to(dev)
    feats = {k: v.to(dev).requires_grad_() for k, v in TS.features(name).items()}
    mask_features, _, multi_scale = pix.forward_features(feats)
    out = dec(multi_scale, mask_features)
    losses = crit(out, targets)
    assert len(losses) == 3 * (3 + 1)
    loss = sum(losses.values())
    assert torch.isfinite(loss)
    loss.backward()
    torch.cuda.synchronize()
    seen = {}
    for k, p in pix.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        seen[_group(k)] = seen.get(_group(k), False) or bool(p.grad.any())
    assert set(seen) == {"attention", "ffn", "norms", "level_embed", "input_proj", "fpn", "mask_features"} and all(seen.values()), seen
    for k, p in dec.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert any(bool(p.grad.any()) for k, p in dec.named_parameters() if "input_proj" in k)
    assert all(v.grad is not None and torch.isfinite(v.grad).all() and bool(v.grad.any()) for v in feats.values())


def test_bench_tool_smoke():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pixel_decoder_train_bench.py"), "--smoke"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "(a) GroupNorm" in r.stdout and "(a) upsample adjoint" in r.stdout and "(b) decoder forward + backward F=2" in r.stdout
