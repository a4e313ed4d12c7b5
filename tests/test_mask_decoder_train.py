"""Training the native mask decoder on the MI355X: the two mask-logit entries alone against fp64 torch at every tile edge, and the
``trainable=True`` modules in ``.train()`` against fp64 autograd of the restated reference (tests/mask_decoder_oracle.py).

Tolerances are those of tests/test_mask_decoder.py: MARGIN = 4 times the PRECISION FLOOR of what is bounded (the same torch operator
sequence in fp32 on the CPU against fp64, never less than one fp32 rounding of the result), computed here from the inputs and never
from the code under test.  The module comparison is teacher-forced with the module's OWN exported attention masks, which are accepted
by that file's rule (``_accept_masks``: decided bits equal, at most CAP of a layer undecided); tests/test_mask_decoder_train_cpu.py
shows that the oracle itself satisfies the condition.  Gradients are bounded per tensor, relative to that tensor's largest magnitude.

The kernel's pixel tile is 64 (MLG_PT, csrc/sf_masklogits.hip); the backward makes one span per tile at these sizes, so P = 131 sums
three partial d_mask_embed in the second pass.

Measured on an MI355X (largest error / bound): forward entry 0.67; backward entry d_me 0.52, d_feat 0.45, accumulated 0.50; module
outputs 0.50 (undecided mask bits 0 in every layer); gradients per group over the three cases: attention 0.54, ffn 0.43, norms 0.50,
class_embed 0.44, mask_embed 0.38, reid_embed 0.29, query_feat 0.28, query_embed 0.42, level_embed 0.32, input_proj 0.32, x 0.34,
mask_features 0.27.
"""
import numpy as np
import pytest
import torch

from tests import mask_decoder_oracle as DO
from tests.helpers import EPS32, MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream, draw as _draw
from tests.test_mask_decoder import CAP, _accept_masks

pytestmark = pytest.mark.gpu

TILE = 64
FR = 2
QS = (1, 5, 16, 17, 100)
PS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)


def _ratio(got, floor32, want):
    bound = MARGIN * fp32_floor(floor32, want)
    return maxabs(got, want) / bound


# ------------------------------------------------------------------------------------------------
# 1. the forward entry alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dm", [4, 64, 256])
def test_forward_entry(Dm):
    nat, dev, worst = _nat(), gpu_device(), 0.0
    for Q in QS:
        for P in PS:
            rs = np.random.RandomState(10000 * Dm + 100 * Q + P)
            me, feat = _draw(rs, FR, Q, Dm), _draw(rs, FR, Dm, P)
            med, fd = me.to(dev), feat.to(dev)
            buf, out = guarded(dev, FR, Q, P)
            nat.check(nat.lib.sf_op_masklogits_forward(med.data_ptr(), fd.data_ptr(), out.data_ptr(), FR, Q, Dm, P, _stream()))
            got = read_guarded(buf, out)
            want = torch.einsum("fqc,fcp->fqp", me.double(), feat.double())
            r = _ratio(got, torch.einsum("fqc,fcp->fqp", me, feat), want)
            worst = max(worst, r)
            assert r <= 1.0, (Q, Dm, P, r)
    print(f"  masklogits forward Dm {Dm}: largest error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------
# 2. the backward entry alone
# ------------------------------------------------------------------------------------------------
def _autograd(me, feat, dl):
    me, feat = me.clone().requires_grad_(), feat.clone().requires_grad_()
    (torch.einsum("fqc,fcp->fqp", me, feat) * dl).sum().backward()
    return me.grad, feat.grad


def _backward(nat, dev, dl, me, feat, want_me=True, want_feat=True, into=None, accumulate=0):
    """-> (d_me, d_feat) on the CPU after the guard checks; ``into``: (buffer, view) of d_feat to add into."""
    Fr, Q, Dm = me.shape
    P = feat.shape[2]
    mbuf, dme = guarded(dev, Fr, Q, Dm)
    fbuf, dfe = into if into is not None else guarded(dev, Fr, Dm, P)
    nbytes = nat.lib.sf_op_masklogits_backward_workspace_bytes(Fr, Q, Dm, P)
    assert nbytes >= Fr * Q * Dm * 4 and nbytes % 256 == 0
    ws = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device=dev)
    nat.check(nat.lib.sf_op_masklogits_backward(dl.data_ptr(), me.data_ptr(), feat.data_ptr(), dme.data_ptr() if want_me else None,
                                                dfe.data_ptr() if want_feat else None, accumulate, Fr, Q, Dm, P, ws.data_ptr() if want_me else None,
                                                nbytes if want_me else 0, _stream()))
    assert (ws[nbytes:].cpu() == 0x5a).all(), "the workspace's guard was written"
    if not want_me:
        assert torch.isnan(mbuf.cpu()).all(), "d_mask_embed was written although NULL was passed"
    if not want_feat:
        assert torch.isnan(fbuf.cpu()).all(), "d_mask_features was written although NULL was passed"
    return (read_guarded(mbuf, dme) if want_me else None), (read_guarded(fbuf, dfe) if want_feat else None)


@pytest.mark.parametrize("Dm", [4, 64, 256])
def test_backward_entry(Dm):
    nat, dev = _nat(), gpu_device()
    worst = dict(d_me=0.0, d_feat=0.0, accumulated=0.0)
    for Q in QS:
        for P in PS:
            rs = np.random.RandomState(20000 * Dm + 100 * Q + P)
            feat = _draw(rs, FR, Dm, P)
            mes, dls = [_draw(rs, FR, Q, Dm) for _ in range(3)], [_draw(rs, FR, Q, P) for _ in range(3)]
            fd, med, dld = feat.to(dev), [t.to(dev) for t in mes], [t.to(dev) for t in dls]
            tag = (Q, Dm, P)
            got_me, got_feat = _backward(nat, dev, dld[0], med[0], fd)
            want = _autograd(mes[0].double(), feat.double(), dls[0].double())
            floor = _autograd(mes[0], feat, dls[0])
            for name, g, f32, w in (("d_me", got_me, floor[0], want[0]), ("d_feat", got_feat, floor[1], want[1])):
                r = _ratio(g, f32, w)
                worst[name] = max(worst[name], r)
                assert r <= 1.0, (tag, name, r)
            # a second run, and either output alone: the same bits
            again = _backward(nat, dev, dld[0], med[0], fd)
            assert torch.equal(again[0], got_me) and torch.equal(again[1], got_feat), (tag, "a second run differs")
            assert torch.equal(_backward(nat, dev, dld[0], med[0], fd, want_feat=False)[0], got_me), (tag, "d_me alone differs")
            assert torch.equal(_backward(nat, dev, dld[0], med[0], fd, want_me=False)[1], got_feat), (tag, "d_feat alone differs")
            # three heads into one buffer
            sums = []
            for _ in range(2):
                into = guarded(dev, FR, Dm, P)
                for i in range(3):
                    d_me_i, acc = _backward(nat, dev, dld[i], med[i], fd, into=into, accumulate=int(i > 0))
                    if i == 0:
                        assert torch.equal(d_me_i, got_me) and torch.equal(acc, got_feat), tag
                sums.append(acc)
            assert torch.equal(sums[0], sums[1]), (tag, "the accumulated gradient differs between two runs")
            want_sum = sum(_autograd(mes[i].double(), feat.double(), dls[i].double())[1] for i in range(3))
            floor_sum = sum(_autograd(mes[i], feat, dls[i])[1] for i in range(3))
            r = _ratio(sums[0], floor_sum, want_sum)
            worst["accumulated"] = max(worst["accumulated"], r)
            assert r <= 1.0, (tag, "accumulated", r)
    print(f"  masklogits backward Dm {Dm}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_entry_refusals():
    nat, dev = _nat(), gpu_device()
    t = torch.zeros(1 << 16, device=dev)
    p = t.data_ptr()
    nbytes = 1 << 17

    def fwd(me=p, feat=p, out=p + (1 << 17), F=2, Q=4, Dm=8, P=8):
        return nat.lib.sf_op_masklogits_forward(me, feat, out, F, Q, Dm, P, _stream())

    def bwd(dl=p, me=p, feat=p, d_me=p + (1 << 16), d_feat=p + (1 << 17), ws=p + (1 << 17) + (1 << 16), ws_bytes=nbytes, F=2, Q=4, Dm=8, P=8):
        return nat.lib.sf_op_masklogits_backward(dl, me, feat, d_me, d_feat, 0, F, Q, Dm, P, ws, ws_bytes, _stream())

    assert fwd() == nat.SF_OK and bwd() == nat.SF_OK
    shapes = (dict(Dm=6), dict(Dm=0), dict(Dm=1028), dict(F=0), dict(F=65536), dict(Q=0), dict(Q=65536), dict(P=0), dict(P=(1 << 24) + 1))
    for kw in (dict(me=None), dict(feat=None), dict(out=None), dict(me=p + 4), dict(feat=p + 8), dict(out=p + 4)) + shapes:
        assert fwd(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_masklogits_forward" in nat.lib.sf_last_error()
    for kw in (dict(dl=None), dict(me=None), dict(feat=None), dict(d_me=None, d_feat=None), dict(ws=None), dict(dl=p + 4), dict(d_me=p + 4),
               dict(d_feat=p + 8), dict(ws=p + 4)) + shapes:
        assert bwd(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_masklogits_backward" in nat.lib.sf_last_error()
    assert bwd(ws_bytes=16) == nat.SF_ERR_WORKSPACE
    big = dict(F=64, Q=8192, Dm=8, P=1 << 13)                  # 2^32 logits
    assert fwd(**big) == nat.SF_ERR_CAPACITY and bwd(**big) == nat.SF_ERR_CAPACITY
    assert nat.lib.sf_op_maskdec_boxes(None, p, 4, 2, 2, _stream()) == nat.SF_ERR_INVALID
    assert nat.lib.sf_op_maskdec_boxes(p, p + 4, 4, 2, 2, _stream()) == nat.SF_ERR_INVALID
    torch.cuda.synchronize()
    assert not t.any()                                         # zeros in: the accepted calls wrote zeros, the refused ones nothing


# ------------------------------------------------------------------------------------------------
# 3. the modules
# ------------------------------------------------------------------------------------------------
PRED_KEYS = ("pred_logits", "pred_masks", "pred_queries", "pred_embeds")


def _module(c, trainable=True):
    import streamformer_amd as sa
    m = getattr(sa, c["cls"])(c["in_channels"], **DO.decoder_kwargs(c), trainable=trainable)
    m.load_state_dict(DO.make_weights(c), strict=True)
    return m.to(gpu_device())


def _cotangents(c, preds):
    """One fixed random cotangent per differentiable output, final and aux: [[tensor per key] per head], fp64 on the CPU."""
    rs = np.random.RandomState(c["seed"] + 99)
    return [{k: torch.from_numpy(rs.standard_normal(tuple(p[k].shape))) for k in PRED_KEYS if k in p} for p in preds]


def _pairing(preds, cots, dtype, dev=None):
    total = 0.0
    for p, ct in zip(preds, cots):
        for k, v in ct.items():
            total = total + (p[k] * v.to(dtype=dtype, device=dev or p[k].device)).sum()
    return total


def _oracle_grads(c, xs, mf, masks, cots, dtype):
    """The forced oracle in ``dtype`` with every weight and input a leaf: (result, {name: grad}) with the inputs as x0, x1, x2 and
    mask_features."""
    sd = {k: v.to(dtype).requires_grad_() for k, v in DO.make_weights(c).items()}
    xs = [x.detach().clone().to(dtype).requires_grad_() for x in xs]      # a copy: .to() of the same dtype is the caller's own tensor
    mf = mf.detach().clone().to(dtype).requires_grad_()
    res = DO.forward(sd, c, xs, mf, dtype=dtype, table="fp64", masks=masks)
    _pairing(res["aux"] + [res], cots, dtype).backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads.update({f"x{l}": x.grad for l, x in enumerate(xs)}, mask_features=mf.grad)
    return res, grads


def _group(name):
    for g in ("self_attn", "multihead_attn", "linear", "norm", "class_embed", "mask_embed", "reid_embed", "query_feat", "query_embed", "level_embed",
              "input_proj", "mask_features"):
        if g in name:
            return {"self_attn": "attention", "multihead_attn": "attention", "linear": "ffn", "norm": "norms"}.get(g, g)
    return "x"


def _run(m, xs, mf, cots=None):
    """One training forward (+ backward with the cotangents) from fresh leaves: (out, {name: grad})."""
    dev = gpu_device()
    m.zero_grad(set_to_none=True)
    xd, mfd = [x.detach().to(dev).requires_grad_() for x in xs], mf.detach().to(dev).requires_grad_()
    out = m(xd, mfd, return_attn_masks=True)
    if cots is None:
        return out, None
    _pairing(out["aux_outputs"] + [out], cots, torch.float32).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({f"x{l}": x.grad for l, x in enumerate(xd)}, mask_features=mfd.grad)
    return out, grads


@pytest.mark.parametrize("name", list(DO.CASES))
def test_module_gradients(name):
    c = DO.CASES[name]
    xs, mf = DO.make_inputs(c, frames=FR)
    m = _module(c).train()
    with torch.no_grad():
        probe = DO.forward(DO.make_weights(c), c, xs, mf, dtype=torch.float32, table="fp64")
    cots = _cotangents(c, probe["aux"] + [probe])
    out, grads = _run(m, xs, mf, cots)
    masks = [t.cpu() for t in out["attn_masks"]]
    assert len(masks) == c["layers"] and len(out["aux_outputs"]) == c["layers"]
    want, want_g = _oracle_grads(c, xs, mf, masks, cots, torch.float64)
    floor, floor_g = _oracle_grads(c, xs, mf, masks, cots, torch.float32)
    for i, packed in enumerate(masks):
        low = want["low_logits"][i].detach()
        band = MARGIN * max(maxabs(floor["low_logits"][i].detach(), low), EPS32 * float(low.abs().max()))
        got = torch.from_numpy(DO.unpack_mask(packed.numpy(), low.shape[-1]))
        share = _accept_masks(f"{name} train layer {i}", got, low < 0, low, band)
        print(f"  {name} train layer {i}: band {band:.3e}, undecided {share:.4f}")
    keys = [k for k in DO.OUTPUTS if k in want and k != "pred_bboxes"]
    assert keys == [k for k in DO.OUTPUTS if k in out and k != "pred_bboxes"]
    for k in keys:
        assert out[k].shape == want[k].shape
        check_against_floor(f"{name} train {k}", out[k].detach(), floor[k].detach(), want[k].detach())
    for i, aux in enumerate(out["aux_outputs"]):
        assert sorted(aux) == sorted(want["aux"][i])
        for k, v in aux.items():
            check_against_floor(f"{name} train aux[{i}].{k}", v.detach(), floor["aux"][i][k].detach(), want["aux"][i][k].detach())
    if DO.is_cl(c):
        pm = want["pred_masks"].detach()
        fband = MARGIN * max(maxabs(floor["pred_masks"].detach(), pm), EPS32 * float(pm.abs().max()))
        sure = ~(pm.abs() <= fband).flatten(2).any(-1)
        assert sure.any() and torch.equal(out["pred_bboxes"].cpu()[sure], want["pred_bboxes"][sure])
        assert torch.equal(out["query_pos_embeds"].cpu(), DO.make_weights(c)["query_embed.weight"][None].expand(FR, -1, -1))
        assert not out["pred_bboxes"].requires_grad and not out["query_pos_embeds"].requires_grad
    assert not any(t.requires_grad for t in out["attn_masks"])
    # gradients: every parameter, every x[l], mask_features
    assert sorted(grads) == sorted(want_g)
    worst = {}
    unreached = [k for k, w in want_g.items() if w is None]      # a level no layer attends to (fewer than three layers): zeros, not None
    assert all("input_proj." in k or k in ("x1", "x2") for k in unreached) and (not unreached or c["layers"] < DO.LEVELS), unreached
    for k in unreached:
        assert grads[k] is not None and not grads[k].any(), (k, "must get a zero gradient")
        del want_g[k]
    for k, w in want_g.items():
        assert grads[k] is not None, (k, "has no gradient")
        assert grads[k].shape == w.shape, k
        r = _ratio(grads[k], floor_g[k], w)
        g = _group(k)
        worst[g] = max(worst.get(g, 0.0), r)
    print(f"  {name} gradients, largest error / bound per group: " + ", ".join(f"{g} {r:.3f}" for g, r in sorted(worst.items())))
    for k, w in want_g.items():
        check_against_floor(f"{name} grad {k}", grads[k], floor_g[k], w)
    # a second forward + backward: the same bits
    out2, grads2 = _run(m, xs, mf, cots)
    for k in keys + (["pred_bboxes"] if DO.is_cl(c) else []):
        assert torch.equal(out2[k], out[k]), k
    for a, b in zip(out2["attn_masks"], out["attn_masks"]):
        assert torch.equal(a, b)
    for k in grads:
        assert torch.equal(grads2[k], grads[k]), (k, "differs between two runs")


@pytest.mark.parametrize("name", list(DO.CASES))
def test_eval_path_is_untouched_and_layer0_masks_agree(name):
    c, dev = DO.CASES[name], gpu_device()
    xs, mf = DO.make_inputs(c, frames=FR)
    xd, mfd = [x.to(dev) for x in xs], mf.to(dev)
    plain, tr = _module(c, trainable=False).eval(), _module(c).eval()
    a, b = plain(xd, mfd, return_aux=True, return_attn_masks=True), tr(xd, mfd, return_aux=True, return_attn_masks=True)
    for k in [k for k in DO.OUTPUTS if k in a] + (["query_pos_embeds"] if DO.is_cl(c) else []):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["aux_outputs"], b["aux_outputs"]):
        assert sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in x)
    assert len(a["attn_masks"]) == c["layers"] and all(torch.equal(x, y) for x, y in zip(a["attn_masks"], b["attn_masks"]))
    with pytest.raises(RuntimeError, match="inference only"):
        plain.train()(xd, mfd)
    # layer 0 attends under the mask of the query table alone: the two paths make the same bits
    out, _ = _run(tr.train(), xs, mf)
    assert torch.equal(out["attn_masks"][0], a["attn_masks"][0])
    tr.trainable = False
    with pytest.raises(RuntimeError, match="inference only"):
        tr(xd, mfd)


# ------------------------------------------------------------------------------------------------
# 4. decoder -> criterion -> backward
# ------------------------------------------------------------------------------------------------
def test_chain_with_the_criterion():
    """The CTVIS decoder's training output goes into SetCriterion (native HungarianMatcher) as it is.  The criterion reads the logits
    and masks only; a plain quadratic term stands in for what CTCLPlugin reads (pred_embeds) so that reid_embed is reached."""
    import streamformer_amd as sa
    c, dev = DO.CASES["cl"], gpu_device()
    xs, mf = DO.make_inputs(c, frames=FR)
    m = _module(c).train()
    H, W = c["mask_grid"]
    targets = []
    for f in range(FR):                                        # two planted targets per frame: the left and the right half
        masks = torch.zeros(2, 2 * H, 2 * W)
        masks[0, :, :W], masks[1, :, W:] = 1.0, 1.0
        targets.append({"labels": torch.tensor([f % c["classes"], (f + 1) % c["classes"]], device=dev), "masks": masks.to(dev)})
    g = torch.Generator(device="cpu").manual_seed(5)
    rand = lambda shape, device: torch.rand(*shape, generator=g).to(device)      # noqa: E731
    crit = sa.SetCriterion(c["classes"], sa.HungarianMatcher(2.0, 5.0, 5.0, num_points=32, rand=rand), {}, 0.1, ["labels", "masks"], 32, 3.0, 0.75,
                           rand=rand).to(dev)
    xd, mfd = [x.to(dev).requires_grad_() for x in xs], mf.to(dev).requires_grad_()
    out = m(xd, mfd)
    losses = crit(out, targets)
    assert len(losses) == 3 * (c["layers"] + 1)
    loss = sum(losses.values()) + sum(p["pred_embeds"].square().mean() for p in out["aux_outputs"] + [out])
    assert torch.isfinite(loss)
    loss.backward()
    torch.cuda.synchronize()
    seen = {}
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        seen[_group(k)] = seen.get(_group(k), False) or bool(p.grad.any())
    want = {"attention", "ffn", "norms", "class_embed", "mask_embed", "reid_embed", "query_feat", "query_embed", "level_embed", "input_proj"}
    assert set(seen) == want and all(seen.values()), seen
    assert all(x.grad is not None and torch.isfinite(x.grad).all() for x in xd + [mfd]) and bool(mfd.grad.any())
