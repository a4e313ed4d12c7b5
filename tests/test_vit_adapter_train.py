"""Training the native ViT-Adapter on the MI355X: the two backward entries alone (DWConv + GELU against fp64 torch autograd, the fuse adjoint
bit for bit against torch's re-layout), and the ``trainable=True`` module in ``.train()`` against fp64 autograd of the training
restatement (tests/vit_adapter_train_support.py, which reproduces fixture F27 of the reference's own class).

Tolerances are the project's: MARGIN = 4 times the PRECISION FLOOR of what is bounded (the same torch operator sequence in fp32 on the CPU
against fp64, never less than one fp32 rounding of the result), computed here from the inputs and never from the code under test.  The
frozen encoder of the floor run has the library's operands (bf16 hi + lo planes), as in tests/test_vit_adapter.py: it runs the same
inference kernels.  Gradients are bounded per tensor.  Two gradients are zero in exact arithmetic, ``up.bias`` and ``spm.fc1.bias`` (each is
added in front of a BatchNorm that subtracts the batch mean): what any implementation holds there is the rounding residue of a cancelling
sum whose summands are those of the same layer's weight gradient, so their bound is that weight gradient's.  The pixels are drawn from
seeds at which no ReLU and no max-pool window of the spatial prior is undecided (tests/test_vit_adapter_train_cpu.py).

Bit-equality of two training steps is claimed for the outputs, for ``level_embed``, ``up.*`` and for every extractor gradient except
``attn.value_proj.*`` and ``feat_norm.*``: with ``feat`` a constant those two are the only ones fed by ``sf_op_msda_backward``'s atomic
grad_value.  The spatial prior's and the final norms' gradients are torch's convolution and BatchNorm backward and are compared against the
bound only.

Measured on an MI355X (largest error / bound): DWConv + GELU backward entry dx 0.23, dw 0.31, db 0.47; module outputs and ``c`` 0.49;
gradients per group over the three cases: attention 0.47, ffn 0.51, norms 0.48, level_embed 0.28, up 0.27, norm1..4 0.42, spm 0.47; running
statistics 0.70.  Two steps gave equal bits for all 99 (sq) / 67 (rect, novit) claimed gradients.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_decoder_oracle as PO
from tests import vit_adapter_oracle as VO
from tests import vit_adapter_train_support as TS
from tests.conftest import ROOT
from tests.helpers import MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream, draw as _draw

pytestmark = pytest.mark.gpu

FR = 2
GRIDS = [(2, 2), (4, 6), (14, 14)]
ZERO_BY_BATCHNORM = {"up.bias": "up.weight", "spm.fc1.bias": "spm.fc1.weight"}


def _ratio(got, floor32, want):
    return maxabs(got, want) / (MARGIN * fp32_floor(floor32, want))


# ------------------------------------------------------------------------------------------------
# 1. DWConv + GELU backward alone
# ------------------------------------------------------------------------------------------------
def _dw_autograd(x, w, b, dy, H, W, dt):
    xt, wt, bt = (t.detach().clone().to(dt).requires_grad_() for t in (x, w, b))
    (F.gelu(VO.dwconv(xt, wt, bt, H, W)) * dy.to(dt)).sum().backward()
    return xt.grad, wt.grad, bt.grad


def _dw_workgroups(nat, Fr, H, W, C_):
    """Partial rows of the weight sums, read off the sizer: the workspace is g rounded up to 256 bytes, then 10 C floats per workgroup."""
    nbytes = nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(Fr, H, W, C_)
    g = (Fr * 21 * (H // 2) * (W // 2) * C_ * 4 + 255) // 256 * 256
    assert nbytes > g and nbytes % 256 == 0
    return (nbytes - g) // (40 * C_)


def _dw_backward(nat, dev, xd, wd, bd, dyd, H, W, want=(True, True, True)):
    """-> (dx, dw, db) on the CPU after the guard checks; an output that is not asked for must stay unwritten."""
    Fr, _, C_ = xd.shape
    bufs = [guarded(dev, *xd.shape), guarded(dev, C_, 1, 3, 3), guarded(dev, C_)]
    nbytes = nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(Fr, H, W, C_)
    ws = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device=dev)
    ptrs = [v.data_ptr() if w else None for (_, v), w in zip(bufs, want)]
    nat.check(nat.lib.sf_op_adapter_dwconv_gelu_backward(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), dyd.data_ptr(), *ptrs, Fr, H, W, C_, ws.data_ptr(),
                                                         nbytes, _stream()))
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


def test_dwconv_backward_shapes_cover_one_and_several_workgroups():
    nat = _nat()
    counts = {(H, W, C_): _dw_workgroups(nat, FR, H, W, C_) for H, W in GRIDS for C_ in (32, 48, 192)}
    assert counts[(2, 2, 32)] == 1 and counts[(14, 14, 192)] > 1, counts


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("C_", [32, 48, 192])
def test_dwconv_gelu_backward_entry(C_, H, W):
    nat, dev = _nat(), gpu_device()
    rs = np.random.RandomState(2700 + C_ + 7 * H + W)
    tokens = 21 * (H // 2) * (W // 2)
    x, w, b = _draw(rs, FR, tokens, C_), _draw(rs, C_, 1, 3, 3) / 3.0, 0.1 * _draw(rs, C_)
    dy = _draw(rs, FR, tokens, C_)
    dy[1] += 1000.0                           # a tap taken across a frame or level boundary shows at once
    xd, wd, bd, dyd = (t.to(dev) for t in (x, w, b, dy))
    got = _dw_backward(nat, dev, xd, wd, bd, dyd, H, W)
    want = _dw_autograd(x, w, b, dy, H, W, torch.float64)
    floor = _dw_autograd(x, w, b, dy, H, W, torch.float32)
    ratios = {k: _ratio(g, f, t) for k, g, f, t in zip(("dx", "dw", "db"), got, floor, want)}
    print(f"  dwconv+gelu backward C={C_} {H}x{W} ({_dw_workgroups(nat, FR, H, W, C_)} workgroups): largest error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, g, f, t in zip(("dx", "dw", "db"), got, floor, want):
        check_against_floor(f"dwconv+gelu backward {k} C={C_} {H}x{W}", g, f, t)
    again = _dw_backward(nat, dev, xd, wd, bd, dyd, H, W)
    assert all(torch.equal(a, g) for a, g in zip(again, got)), "a second run differs"
    for i, key in enumerate(("dx", "dw", "db")):
        alone = _dw_backward(nat, dev, xd, wd, bd, dyd, H, W, want=tuple(j == i for j in range(3)))
        assert torch.equal(alone[i], got[i]), (key, "alone differs from the joint run")


# ------------------------------------------------------------------------------------------------
# 2. the fuse adjoint alone: a permutation has no tolerance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", GRIDS + [(10, 26)])
@pytest.mark.parametrize("D", [8, 64, 72, 96])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_fuse_backward_entry(level, D, H, W):
    nat, dev = _nat(), gpu_device()
    Ho, Wo = ((4 * H, 4 * W), (2 * H, 2 * W), (H, W), (H // 2, W // 2))[level]
    dy = _draw(np.random.RandomState(2750 + level + 5 * D + 7 * H + W), FR, D, Ho, Wo)
    dyd = dy.to(dev)
    n = (H // 2) * (W // 2)
    if level == 0:
        buf, out = guarded(dev, FR * 16 * n, 4 * D)
        nat.check(nat.lib.sf_op_adapter_fuse_backward(0, dyd.data_ptr(), out.data_ptr(), 16 * n * 4 * D, FR, H, W, D, _stream()))
        torch.cuda.synchronize()
        want = dy.reshape(FR, D, 2 * H, 2, 2 * W, 2).permute(0, 2, 4, 3, 5, 1).reshape(FR * 16 * n, 4 * D)      # the inverse pixel shuffle
        assert torch.equal(read_guarded(buf, out), want)
        return
    buf, out = guarded(dev, FR, 21 * n, D)
    out.fill_(7.0)
    lo, hi = ((0, 16 * n), (16 * n, 20 * n), (20 * n, 21 * n))[level - 1]
    assert hi - lo == Ho * Wo
    nat.check(nat.lib.sf_op_adapter_fuse_backward(level, dyd.data_ptr(), out.data_ptr() + 4 * lo * D, 21 * n * D, FR, H, W, D, _stream()))
    torch.cuda.synchronize()
    got = read_guarded(buf, out)
    assert torch.equal(got[:, lo:hi], dy.flatten(2).transpose(1, 2))
    assert (got[:, :lo] == 7.0).all() and (got[:, hi:] == 7.0).all(), "another level's slice was written"


# ------------------------------------------------------------------------------------------------
# 3. refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refusals():
    nat, dev = _nat(), gpu_device()
    t = torch.zeros(1 << 16, device=dev)
    p = t.data_ptr()
    K = 1 << 10

    def dw(x=p, w=p, b=p, dy=p + 16 * K, dx=p + 64 * K, dwt=p + 128 * K, db=p + 129 * K, ws=p + 192 * K, ws_bytes=32 * K, F_=2, H=2, W=2, C_=32):
        return nat.lib.sf_op_adapter_dwconv_gelu_backward(x, w, b, dy, dx, dwt, db, F_, H, W, C_, ws, ws_bytes, _stream())

    def fuse(level=1, dy=p, d_tok=p + 64 * K, stride=21 * 8, F_=2, H=2, W=2, D=8):
        return nat.lib.sf_op_adapter_fuse_backward(level, dy, d_tok, stride, F_, H, W, D, _stream())

    assert dw() == nat.SF_OK and fuse() == nat.SF_OK and fuse(level=0, stride=16 * 32) == nat.SF_OK and fuse(level=3) == nat.SF_OK
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(dy=None), dict(ws=None), dict(dx=None, dwt=None, db=None), dict(x=p + 4), dict(b=p + 8),
               dict(dy=p + 16 * K + 12), dict(dx=p + 64 * K + 4), dict(ws=p + 192 * K + 16), dict(dx=p), dict(dx=p + 16 * K), dict(F_=0), dict(H=3), dict(W=3),
               dict(H=0), dict(W=1), dict(C_=0), dict(C_=30), dict(C_=1028), dict(C_=-4)):
        assert dw(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_adapter_dwconv_gelu_backward" in nat.lib.sf_last_error()
    assert dw(ws_bytes=256) == nat.SF_ERR_WORKSPACE and b"workspace" in nat.lib.sf_last_error()
    assert dw(F_=65535, H=256, W=256, C_=1024) == nat.SF_ERR_CAPACITY
    assert nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(65535, 256, 256, 1024) == 0
    assert nat.lib.sf_op_adapter_dwconv_gelu_backward_workspace_bytes(2, 3, 2, 32) == 0
    for kw in (dict(level=-1), dict(level=4), dict(dy=None), dict(d_tok=None), dict(d_tok=p + 64 * K + 8), dict(F_=0), dict(F_=65536), dict(H=0), dict(W=0),
               dict(H=4097), dict(level=3, H=3, stride=21 * 8 * 4), dict(D=0), dict(D=6), dict(stride=16 * 8 - 4), dict(stride=21 * 8 + 2),
               dict(level=0, stride=16 * 32 - 4)):
        assert fuse(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_adapter_fuse_backward" in nat.lib.sf_last_error()
    torch.cuda.synchronize()
    assert not t.any()                                         # zeros in: the accepted calls wrote zeros, the refused ones nothing


# ------------------------------------------------------------------------------------------------
# 4. the module
# ------------------------------------------------------------------------------------------------
def _module(name, trainable=True, sd=None):
    import streamformer_amd as sa
    c = VO.CASES[name]
    m = sa.TimesformerMultiTaskingModelSigLIPViTAdapter(VO.config(c), **VO.adapter_kwargs(c), trainable=trainable)
    m.load_state_dict(TS.weights(name) if sd is None else sd, strict=True)
    return m.to(gpu_device())


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(fp64 run, its gradients, fp32 floor run, its gradients, the cotangents): computed once per case, read only."""
    want, floor = TS.Run(name, torch.float64), TS.Run(name, torch.float32, encoder_operands="x3")
    cots = TS.cotangents(name, want.outs)
    return want, want.backward(cots), floor, floor.backward(cots), cots


def _group(name):
    for g, label in (("spm.", "spm"), ("level_embed", "level_embed"), (".attn.", "attention"), (".ffn.", "ffn"), ("_norm.", "norms"), ("up.", "up"),
                     ("norm", "norm1..4")):
        if g in name:
            return label
    raise AssertionError(name)


def _claimed_bit_equal(name):
    if name == "level_embed" or name.startswith("up."):
        return True
    return name.startswith("interactions.") and ".attn.value_proj." not in name and ".feat_norm." not in name


def _step(m, name, cots):
    dev = gpu_device()
    m.zero_grad(set_to_none=True)
    outs, c = m.forward_with_tokens(TS.pixels(name).to(dev))
    TS.pairing(outs, cots, torch.float32).backward()
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in outs.items()}, c.detach(), {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(VO.CASES))
def test_module_gradients(name):
    want, want_g, floor, floor_g, cots = _oracle(name)
    m = _module(name).train()
    before = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    outs, c, grads = _step(m, name, cots)
    assert list(outs) == list(VO.OUTPUTS)
    for k in VO.OUTPUTS:
        assert outs[k].shape == want.outs[k].shape and outs[k].dtype == torch.float32
        check_against_floor(f"{name} train {k}", outs[k], floor.outs[k].detach(), want.outs[k].detach())
    check_against_floor(f"{name} train c", c, floor.c.detach(), want.c.detach())
    # the frozen backbone has no gradient, every learned parameter has one of its own shape inside its bound
    learned = set(want_g)
    assert {k for k, g in grads.items() if g is not None} == learned
    assert all(grads[k] is None for k in grads if k.startswith(TS.BACKBONE))
    worst = {}
    for k, w in want_g.items():
        assert grads[k].shape == w.shape, k
        ref = ZERO_BY_BATCHNORM.get(k)
        bound = MARGIN * (fp32_floor(floor_g[k], w) if ref is None else max(fp32_floor(floor_g[ref], want_g[ref]), fp32_floor(floor_g[k], w)))
        worst[_group(k)] = max(worst.get(_group(k), 0.0), maxabs(grads[k], w) / bound)
    print(f"  {name} gradients, largest error / bound per group: " + ", ".join(f"{g} {r:.3f}" for g, r in sorted(worst.items())))
    for k, w in want_g.items():
        ref = ZERO_BY_BATCHNORM.get(k)
        bound = MARGIN * (fp32_floor(floor_g[k], w) if ref is None else max(fp32_floor(floor_g[ref], want_g[ref]), fp32_floor(floor_g[k], w)))
        err = maxabs(grads[k], w)
        assert err <= bound, (name, k, err, bound)
    # the running statistics have moved, inside the floor
    sd = m.state_dict()
    for k, w in want.stats.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(w) == int(before[k]) + 1
        else:
            assert not torch.equal(sd[k], before[k]), (k, "did not move")
            check_against_floor(f"{name} {k}", sd[k], floor.stats[k], w)
    # a second forward + backward from the same state: the same bits where no float atomic is passed
    m.load_state_dict({**m.state_dict(), **before}, strict=True)
    outs2, c2, grads2 = _step(m, name, cots)
    assert all(torch.equal(outs2[k], outs[k]) for k in outs) and torch.equal(c2, c)
    fixed = [k for k in learned if _claimed_bit_equal(k)]
    assert len(fixed) >= 40
    moved = [k for k in fixed if not torch.equal(grads2[k], grads[k])]
    print(f"  {name}: {len(fixed)} gradients claimed bit-equal; of the others, equal in this run: "
          f"{sum(torch.equal(grads2[k], grads[k]) for k in learned if k not in fixed)} of {len(learned) - len(fixed)}")
    assert not moved, (moved, "differ between two runs")


# ------------------------------------------------------------------------------------------------
# 5. eval untouched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VO.CASES))
def test_eval_path_is_untouched(name):
    dev = gpu_device()
    px = TS.pixels(name).to(dev)
    plain, tr = _module(name, trainable=False).eval(), _module(name).eval()
    a, b = plain.forward_with_tokens(px), tr.forward_with_tokens(px)
    assert all(torch.equal(a[0][k], b[0][k]) for k in VO.OUTPUTS) and torch.equal(a[1], b[1])
    assert not any(t.requires_grad for t in list(b[0].values()) + [b[1]])
    with pytest.raises(NotImplementedError, match="inference only.*trainable=True"):
        plain.train()(px)
    tr.trainable = False
    with pytest.raises(NotImplementedError, match="inference only"):
        tr.train()(px)


def test_eval_after_a_training_step_refolds_the_tail():
    """The running statistics moved and an optimiser stepped: the next eval() forward must fold the tail again (_folded_tail's token covers
    the norms' tensors).  A fresh module loaded from the trained state dict is the witness."""
    name, dev = "sq", gpu_device()
    px = TS.pixels(name).to(dev)
    m = _module(name).eval()
    first = m(px)
    m.train()
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    outs = m(px)
    sum(v.square().mean() for v in outs.values()).backward()
    opt.step()
    got = m.eval()(px)
    fresh = _module(name, trainable=False, sd=m.state_dict()).eval()(px)
    assert all(torch.equal(got[k], fresh[k]) for k in VO.OUTPUTS)
    assert not any(torch.equal(got[k], first[k]) for k in VO.OUTPUTS)


# ------------------------------------------------------------------------------------------------
# 6. adapter -> pixel decoder -> mask decoder -> criterion -> backward
# ------------------------------------------------------------------------------------------------
def test_chain_from_the_adapter_to_the_criterion():
    import streamformer_amd as sa
    name, dev = "sq", gpu_device()
    D, (Hg, Wg) = VO.CASES[name]["hidden"], VO.grid(VO.CASES[name])
    classes = 5
    adapter = _module(name).train()
    pc = dict(channels=(D,) * 4, grids=[(4 * Hg, 4 * Wg), (2 * Hg, 2 * Wg), (Hg, Wg), (Hg // 2, Wg // 2)], transformer=("res3", "res4", "res5"), conv_dim=64,
              heads=8, ffn=128, mask_dim=64, layers=2, seed=2790)
    shape = {k: sa.ShapeSpec(ch, s) for k, ch, s in zip(PO.LEVELS, pc["channels"], PO.STRIDES)}
    pix = sa.MSDeformAttnPixelDecoder(shape, **PO.decoder_kwargs(pc), trainable=True)
    pix.load_state_dict(PO.make_weights(pc), strict=True)
    pix = pix.to(dev).train()
    torch.manual_seed(2791)
    dec = sa.MultiScaleMaskedTransformerDecoder(pc["conv_dim"], num_classes=classes, hidden_dim=64, num_queries=8, nheads=4, dim_feedforward=128, dec_layers=3,
                                                pre_norm=False, mask_dim=pc["mask_dim"], enforce_input_project=True, trainable=True).to(dev).train()
    H, W = pc["grids"][0]
    targets = []
    for f in range(FR):                                        # two planted targets per frame: the left and the right half
        masks = torch.zeros(2, 2 * H, 2 * W)
        masks[0, :, :W], masks[1, :, W:] = 1.0, 1.0
        targets.append({"labels": torch.tensor([f % classes, (f + 1) % classes], device=dev), "masks": masks.to(dev)})
    g = torch.Generator(device="cpu").manual_seed(5)
    rand = lambda shape, device: torch.rand(*shape, generator=g).to(device)      # noqa: E731
    crit = sa.SetCriterion(classes, sa.HungarianMatcher(2.0, 5.0, 5.0, num_points=32, rand=rand), {}, 0.1, ["labels", "masks"], 32, 3.0, 0.75,
                           rand=rand).to(dev)
    feats = adapter(TS.pixels(name).to(dev))
    assert all(v.requires_grad for v in feats.values())
    mask_features, _, multi_scale = pix.forward_features(dict(feats))
    losses = crit(dec(multi_scale, mask_features), targets)
    loss = sum(losses.values())
    assert torch.isfinite(loss)
    loss.backward()
    torch.cuda.synchronize()
    seen = {}
    for k, p in adapter.named_parameters():
        if k.startswith(TS.BACKBONE):
            assert p.grad is None, k
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        label = _group(k)
        if label in ("attention", "ffn", "norms"):
            label = k[:k.index(".attn." if ".attn." in k else ".ffn." if ".ffn." in k else "." + k.split(".")[-2] + ".")] + ":" + label
        seen[label] = seen.get(label, False) or bool(p.grad.any())
    extractors = [p[:-1] for block in VO.extractor_prefixes(VO.CASES[name]) for p in block]
    assert set(seen) == {"spm", "level_embed", "up", "norm1..4"} | {f"{e}:{g}" for e in extractors for g in ("attention", "ffn", "norms")}, sorted(seen)
    assert all(seen.values()), seen
    for n in (adapter.norm1, adapter.norm2, adapter.norm3, adapter.norm4):
        assert bool(n.weight.grad.any()) and bool(n.bias.grad.any())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in list(pix.parameters()) + list(dec.parameters()))


def test_bench_tool_smoke():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vit_adapter_train_bench.py"), "--smoke"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "(a) DWConv+GELU backward" in r.stdout and "(a) fuse adjoint" in r.stdout and "(b) adapter forward + backward" in r.stdout
