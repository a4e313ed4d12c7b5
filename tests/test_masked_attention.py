"""Masked attention for training on the MI355X: the forward with statistics, the backward kernels and the packer alone, then the module
and use_native_attention against fp64 nn.MultiheadAttention.

Oracle: torch autograd in fp64 on the CPU through the plain sequence (tests/masked_attention_oracle.py; the module tests use
nn.MultiheadAttention itself).  Every bound is MARGIN = 4 times the precision floor (tests/helpers.check_against_floor): the error of
the same sequence in fp32 torch against fp64, at least one fp32 rounding of the result.  Two frames everywhere, two heads in the kernel
tests.  The mask words given to the kernels have their padding bits CLEAR (tests/mask_decoder_oracle.pack_mask), so a kernel that
trusted them would see keys past HW; one more run sets them at random and must give the same bits.

Measured on an MI355X, largest error / bound over all cases: stats 0.42, dq 0.78, dk 0.66, dv 0.39 (the two largest at head width 8);
module 0.39, the swapped layer 0.36.
"""
import numpy as np
import pytest
import torch
from torch import nn

from tests import mask_decoder_oracle as DO
from tests import masked_attention_oracle as MO
from tests.helpers import MARGIN, check_against_floor, fp32_floor, gpu_device, guarded, maxabs, read_guarded
from tests.helpers import native as _nat, stream as _stream

pytestmark = pytest.mark.gpu

FR, HEADS = 2, 2
# (head width, Q, HW): every value of each axis at least once, the smallest and the largest of all three together
CASES = [(8, 1, 1), (32, 15, 15), (32, 16, 16), (72, 17, 17), (32, 16, 31), (8, 17, 32), (72, 15, 33), (32, 100, 63), (8, 16, 64),
         (128, 17, 65), (72, 100, 100), (128, 100, 784)]


def _ma():
    import streamformer_amd as ma      # the package exports the whole interface (its attribute masked_attention is the function)
    return ma


def _ratio(what, got, floor32, want):
    if fp32_floor(floor32, want) == 0.0:      # an exactly zero gradient (one visible key per query: softmax's backward cancels) has a zero bound
        assert not got.any(), (what, "must be exactly zero")
        return 0.0
    check_against_floor(what, got, floor32, want)
    return maxabs(got, want) / (MARGIN * fp32_floor(floor32, want))


def _words(m, dev, rs=None):
    """numpy bool mask -> device words with clear padding bits, or (rs given) random ones"""
    if m is None:
        return None
    w = DO.pack_mask(m)
    HW = m.shape[-1]
    if rs is not None and HW % 32:
        junk = rs.randint(0, 2 ** 31, size=w.shape[:-1]).astype(np.uint32) << np.uint32(HW % 32)
        w = w.copy()
        w[..., -1] = (w[..., -1].view(np.uint32) | junk).view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(w)).to(dev)


def _forward(q, qp, k, v, kvp, words, per_head, Q, HW, hd, want_stats=True, no_skip=0):
    nat, dev = _nat(), gpu_device()
    buf, out = guarded(dev, FR, Q, HEADS * hd)
    sbuf, stats = guarded(dev, FR, HEADS, Q)
    nat.check(nat.lib.sf_op_maskattn_forward(q, qp, k, v, kvp, nat.ptr(words), per_head, out.data_ptr(), stats.data_ptr() if want_stats else None,
                                             FR, Q, HW, HEADS, hd, no_skip, _stream()))
    return read_guarded(buf, out), (read_guarded(sbuf, stats) if want_stats else None), out, stats


def _backward(q, qp, k, v, kvp, words, per_head, ctx, stats, do, Q, HW, hd, no_skip=0):
    nat, dev, D = _nat(), gpu_device(), HEADS * hd
    bufs = [guarded(dev, FR, T, D) for T in (Q, HW, HW)]
    nat.check(nat.lib.sf_op_maskattn_backward(q, qp, k, v, kvp, nat.ptr(words), per_head, ctx.data_ptr(), stats.data_ptr(), do.data_ptr(),
                                              bufs[0][1].data_ptr(), D, bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), D, FR, Q, HW, HEADS, hd,
                                              no_skip, _stream()))
    return [read_guarded(b, o) for b, o in bufs]


@pytest.mark.parametrize("hd,Q,HW", CASES)
def test_kernels(hd, Q, HW):
    nat, dev, D = _nat(), gpu_device(), HEADS * hd
    rs = np.random.RandomState(100000 * hd + 1000 * Q + HW)
    draw = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))      # noqa: E731
    q, k, v, do = draw(FR, Q, D), draw(FR, HW, D), draw(FR, HW, D), draw(FR, Q, D)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    qb, kvb = torch.randn(FR, Q, 3 * D, device=dev), torch.randn(FR, HW, 3 * D, device=dev)      # column ranges of [rows, 3 D] buffers
    qb[..., D:2 * D], kvb[..., :D], kvb[..., 2 * D:] = qd, kd, vd
    pitched = (qb.data_ptr() + 4 * D, 3 * D, kvb.data_ptr(), kvb.data_ptr() + 8 * D, 3 * D)
    worst = dict(stats=0.0, dq=0.0, dk=0.0, dv=0.0)
    for kind in MO.MASKS:
        m = MO.make_mask(kind, rs, FR, HEADS, Q, HW)
        per_head = int(kind == "heads")
        words = _words(m, dev)
        tag = f"hd {hd} Q {Q} HW {HW} {kind}"
        # ---- forward: ctx bit-equal to the decoder's kernel, with and without the statistics ----
        ctx, stats, ctx_d, stats_d = _forward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, words, per_head, Q, HW, hd)
        plain = _forward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, words, per_head, Q, HW, hd, want_stats=False)[0]
        assert torch.equal(ctx, plain), (tag, "ctx changes with the statistics")
        for h in range(HEADS if per_head else 1):
            buf, out = guarded(dev, FR, Q, D)
            wh = None if words is None else (words[:, h].contiguous() if per_head else words)
            nat.check(nat.lib.sf_op_maskdec_attention(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, None, 0, nat.ptr(wh), out.data_ptr(), None, None,
                                                      FR, Q, HW, HEADS, hd, 0, _stream()))
            cols = slice(h * hd, (h + 1) * hd) if per_head else slice(None)
            assert torch.equal(read_guarded(buf, out)[..., cols], ctx[..., cols]), (tag, "ctx differs from sf_op_maskdec_attention")
        want = MO.autograd_backward(q.double(), k.double(), v.double(), m, HEADS, do.double())
        floor = MO.autograd_backward(q, k, v, m, HEADS, do)
        dead = torch.isinf(want[1])
        assert torch.equal(torch.isinf(stats) & (stats > 0), dead), (tag, "+inf statistics exactly where no key is visible")
        if not dead.all():
            live = lambda t: t.masked_fill(dead, 0.0)      # noqa: E731
            worst["stats"] = max(worst["stats"], _ratio(tag + " stats", live(stats), live(floor[1]), live(want[1])))
        # ---- backward ----
        got = _backward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, words, per_head, ctx_d, stats_d, dod, Q, HW, hd)
        for i, name in enumerate(("dq", "dk", "dv")):
            worst[name] = max(worst[name], _ratio(f"{tag} {name}", got[i], floor[2 + i], want[2 + i]))
        hm = MO.head_mask(m, FR, HEADS, Q, HW)
        blind = hm.all(-1)[..., None].expand(FR, HEADS, Q, hd)             # (frame, head, query) that sees no key
        unseen = hm.all(-2)[..., None].expand(FR, HEADS, HW, hd)           # (frame, head, key) that no query sees
        assert not MO.split(got[0], HEADS)[blind].any() and not MO.split(ctx, HEADS)[blind].any(), (tag, "a blind query's dq / ctx are not zero")
        assert not MO.split(got[1], HEADS)[unseen].any() and not MO.split(got[2], HEADS)[unseen].any(), (tag, "an unseen key's dk / dv are not zero")
        if kind in ("query", "heads"):
            assert blind.any()
        if kind in ("key", "heads", "last"):
            assert unseen.any() or HW == 1
        # ---- the same bits: unskipped, again, pitched operands, garbage in the padding bits ----
        runs = {"no_skip": _backward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, words, per_head, ctx_d, stats_d, dod, Q, HW, hd, no_skip=1),
                "second run": _backward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, words, per_head, ctx_d, stats_d, dod, Q, HW, hd),
                "pitched": _backward(*pitched, words, per_head, ctx_d, stats_d, dod, Q, HW, hd)}
        if words is not None and HW % 32:
            junk = _words(m, dev, rs)
            assert not torch.equal(junk, words)
            runs["padding bits"] = _backward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, junk, per_head, ctx_d, stats_d, dod, Q, HW, hd)
            fj = _forward(qd.data_ptr(), D, kd.data_ptr(), vd.data_ptr(), D, junk, per_head, Q, HW, hd)
            assert torch.equal(fj[0], ctx) and torch.equal(fj[1], stats), (tag, "the forward reads the padding bits")
        for name, other in runs.items():
            for a, b_, n in zip(got, other, ("dq", "dk", "dv")):
                assert torch.equal(a, b_), (tag, name, n, "differs")
        fp = _forward(*pitched, words, per_head, Q, HW, hd, no_skip=1)
        assert torch.equal(fp[0], ctx) and torch.equal(fp[1], stats), (tag, "the forward with pitches / unskipped differs")
    print(f"  hd {hd} Q {Q} HW {HW}: largest error / bound " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))


def test_kernel_refusals():
    nat, dev = _nat(), gpu_device()
    t = torch.zeros(4096, device=dev)
    p = t.data_ptr()

    def bwd(q=p, ctx=p, dq=p, F=2, Q=4, HW=8, hd=8, pitch=16):
        return nat.lib.sf_op_maskattn_backward(q, pitch, p, p, pitch, None, 0, ctx, p, p, dq, pitch, p, p, pitch, F, Q, HW, 2, hd, 0, _stream())

    assert bwd() == nat.SF_OK
    for kw in (dict(q=None), dict(ctx=None), dict(dq=None), dict(q=p + 4), dict(dq=p + 8), dict(hd=12), dict(hd=136), dict(F=0), dict(F=65536),
               dict(Q=0), dict(HW=0), dict(HW=(1 << 24) + 1), dict(pitch=8), dict(pitch=18)):
        assert bwd(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_maskattn_backward" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_maskattn_forward(p + 4, 16, p, p, 16, None, 0, p, p, 2, 4, 8, 2, 8, 0, _stream()) == nat.SF_ERR_INVALID

    def dec(F=2, Q=4, HW=8, heads=2):                        # the decoder's entry point has the bounds of the other two
        return nat.lib.sf_op_maskdec_attention(p, 16, p, p, 16, None, 0, None, p, None, None, F, Q, HW, heads, 8, 0, _stream())

    assert dec() == nat.SF_OK
    for kw in (dict(F=65536), dict(Q=65536), dict(HW=(1 << 24) + 1), dict(heads=65536), dict(F=0), dict(Q=0), dict(HW=0), dict(heads=0)):
        assert dec(**kw) == nat.SF_ERR_INVALID, kw
        assert b"sf_op_maskdec_attention" in nat.lib.sf_last_error()
    assert nat.lib.sf_op_maskattn_pack(None, p, 4, 8, _stream()) == nat.SF_ERR_INVALID
    assert nat.lib.sf_op_maskattn_pack(p, p, 4, 0, _stream()) == nat.SF_ERR_INVALID
    torch.cuda.synchronize()
    assert not t.any()                                       # ctx = d_ctx = 0: the accepted call wrote zeros, the refused ones nothing


@pytest.mark.parametrize("HW", [1, 15, 31, 32, 33, 63, 64, 65, 100, 784])
def test_pack(HW):
    ma, dev = _ma(), gpu_device()
    rs = np.random.RandomState(HW)
    for shape in ((2, 5, HW), (2, 3, 5, HW)):
        m = rs.random_sample(shape) < 0.5
        padded = np.concatenate([m, np.ones(shape[:-1] + ((-HW) % 32,), bool)], -1)      # the padding bits are set
        got = ma.pack_attention_mask(torch.from_numpy(m).to(dev))
        assert got.HW == HW and got.per_head == (len(shape) == 4)
        assert np.array_equal(got.words.cpu().numpy(), DO.pack_mask(padded)), shape
    flat = ma.pack_attention_mask(torch.from_numpy(m.reshape(6, 5, HW)).to(dev), heads=3)      # [F * heads, Q, HW], head-minor
    assert flat.per_head and torch.equal(flat.words, got.words)


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
def _module_case(kind, C=64, heads=4, Q=20, HW=40, seed=0):
    """-> the inputs, the mask as torch takes it, and fp64 / fp32 nn.MultiheadAttention results: out, input and parameter gradients"""
    torch.manual_seed(seed)
    ref = nn.MultiheadAttention(C, heads)
    with torch.no_grad():
        ref.in_proj_bias.normal_(0, 0.1)
        ref.out_proj.bias.normal_(0, 0.1)
    x = torch.randn(Q, FR, C)
    y, z = (x, x) if kind == "self" else (torch.randn(HW, FR, C), torch.randn(HW, FR, C))
    g = torch.randn(Q, FR, C)
    mask = None
    if kind != "self":
        mask = torch.rand(FR * heads if kind == "per_head" else FR, Q, HW) < 0.6
        mask[..., 3] = False                                 # torch gives NaN for a fully hidden row
        if kind == "per_head":
            assert not torch.equal(mask[0], mask[1])

    def run(dtype):
        mod = nn.MultiheadAttention(C, heads).to(dtype)
        mod.load_state_dict({k_: v_.to(dtype) for k_, v_ in ref.state_dict().items()})
        ins = [t.detach().to(dtype).clone().requires_grad_(True) for t in ((x,) if kind == "self" else (x, y, z))]
        m = mask if mask is None or kind == "per_head" else mask.repeat_interleave(heads, 0)
        out = mod(*(ins * 3 if kind == "self" else ins), attn_mask=m, need_weights=False)[0]
        out.backward(g.to(dtype))
        return [out.detach()] + [t.grad for t in ins] + [p.grad for p in mod.parameters()]

    return ref, (x, y, z), g, mask, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("kind", ["per_head", "shared", "self"])
def test_module_against_multihead_attention(kind):
    ma, dev = _ma(), gpu_device()
    ref, (x, y, z), g, mask, want, floor = _module_case(kind)

    def run(attn_mask):
        mod = ma.MaskedMultiheadAttention(ref.embed_dim, ref.num_heads).to(dev)
        mod.load_state_dict(ref.state_dict(), strict=True)
        ins = [t.detach().to(dev).requires_grad_(True) for t in ((x,) if kind == "self" else (x, y, z))]
        out, weights = mod(*(ins * 3 if kind == "self" else ins), attn_mask=attn_mask)
        assert weights is None and tuple(out.shape) == tuple(x.shape)
        out.backward(g.to(dev))
        return [out.detach().cpu()] + [t.grad.cpu() for t in ins] + [p.grad.cpu() for p in mod.parameters()]

    got = run(None if mask is None else mask.to(dev))
    names = ["out"] + ["d_query", "d_key", "d_value"][:len(got) - 5] + ["d_in_proj_weight", "d_in_proj_bias", "d_out_proj.weight", "d_out_proj.bias"]
    worst = max(_ratio(f"{kind} {n}", a, f, w) for n, a, f, w in zip(names, got, floor, want))
    print(f"  module {kind}: largest error / bound {worst:.3f}")
    if mask is not None:
        packed = ma.pack_attention_mask(mask.to(dev), heads=ref.num_heads if kind == "per_head" else None)
        assert packed.per_head == (kind == "per_head")
        for n, a, b in zip(names, got, run(packed)):
            assert torch.equal(a, b), (n, "differs with a PackedAttentionMask")
    if kind == "shared":                                     # a [Tq, Tk] mask is the same mask in every frame
        two = mask[0].to(dev)
        mod = ma.MaskedMultiheadAttention(ref.embed_dim, ref.num_heads).to(dev)
        mod.load_state_dict(ref.state_dict())
        with torch.no_grad():
            a = mod(x.to(dev), y.to(dev), z.to(dev), attn_mask=two)[0]
            b = mod(x.to(dev), y.to(dev), z.to(dev), attn_mask=two[None].expand(FR, -1, -1))[0]
        assert torch.equal(a, b)


def test_fully_hidden_row_gives_zeros():
    ma, dev = _ma(), gpu_device()
    torch.manual_seed(1)
    q, k, v = (torch.randn(FR, T, 32, device=dev, requires_grad=True) for T in (5, 9, 9))
    mask = torch.zeros(FR, 5, 9, dtype=torch.bool, device=dev)
    mask[:, 2] = True
    out = ma.masked_attention(q, k, v, ma.pack_attention_mask(mask), heads=4)
    out.sum().backward()
    assert not out[:, 2].any() and not q.grad[:, 2].any() and torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all()


def test_use_native_attention():
    ma, dev = _ma(), gpu_device()

    class Layer(nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn = nn.MultiheadAttention(32, 4)
            self.multihead_attn = nn.MultiheadAttention(32, 4)
            self.norm = nn.LayerNorm(32)

        def forward(self, tgt, memory, mask):
            tgt = tgt + self.self_attn(tgt, tgt, tgt)[0]
            return self.norm(tgt + self.multihead_attn(tgt, memory, memory, attn_mask=mask)[0])

    torch.manual_seed(2)
    net = Layer()
    tgt, memory, g = torch.randn(6, FR, 32), torch.randn(21, FR, 32), torch.randn(6, FR, 32)
    mask = torch.rand(FR * 4, 6, 21) < 0.5
    mask[..., 0] = False

    def grads(model, dtype, where):
        model = model.to(dtype).to(where)
        model.zero_grad()
        out = model(tgt.to(dtype).to(where), memory.to(dtype).to(where), mask.to(where))
        out.backward(g.to(dtype).to(where))
        return [out.detach().cpu()] + [p.grad.cpu().clone() for p in model.parameters()]

    import copy
    want = grads(copy.deepcopy(net), torch.float64, "cpu")
    floor = grads(copy.deepcopy(net), torch.float32, "cpu")
    before = {k_: v_.clone() for k_, v_ in net.state_dict().items()}
    assert ma.use_native_attention(net) == 2
    assert isinstance(net.self_attn, ma.MaskedMultiheadAttention) and isinstance(net.multihead_attn, ma.MaskedMultiheadAttention)
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k_], before[k_]) for k_ in before)
    got = grads(net, torch.float32, dev)
    names = ["out"] + [n for n, _ in net.named_parameters()]
    for n, a, f, w in zip(names, got, floor, want):
        check_against_floor("swapped layer " + n, a, f, w)
