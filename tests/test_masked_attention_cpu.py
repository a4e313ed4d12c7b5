"""Masked attention for training, the parts that need no GPU: the fp64 restatement of the recompute-from-statistics backward against
torch autograd, the module's parameter tree against nn.MultiheadAttention, every refusal, and the packed layout.

The restatement and autograd differ by fp64 rounding only: the bound is 1e-12 of the case's largest gradient entry."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import mask_decoder_oracle as DO
from tests import masked_attention_oracle as MO


def _ma():
    import streamformer_amd as ma      # the package exports the whole interface (its attribute masked_attention is the function)
    return ma


@pytest.mark.parametrize("kind", MO.MASKS)
def test_restatement_equals_autograd(kind):
    Fr, heads, hd, Q, HW = 2, 2, 8, 17, 45
    rs = np.random.RandomState(11)
    q, k, v, do = (torch.from_numpy(rs.standard_normal((Fr, T, heads * hd))) for T in (Q, HW, HW, Q))
    m = MO.make_mask(kind, rs, Fr, heads, Q, HW)
    ctx, stats, dq, dk, dv = MO.autograd_backward(q, k, v, m, heads, do)
    got = MO.recompute_backward(q, k, v, m, heads, ctx, stats, do)
    top = max(float(w.abs().max()) for w in (dq, dk, dv))      # one scale for the three: "last" has dq = dk = 0 but for rounding
    for name, g, w in zip(("dq", "dk", "dv"), got, (dq, dk, dv)):
        rel = float((g - w).abs().max()) / top
        print(f"  {kind} {name}: {rel:.2e}")
        assert rel <= 1e-12, (kind, name, rel)
    if kind == "query":       # a fully hidden row: +inf statistics, zero output, zero dq
        assert torch.isinf(stats[:, :, Q // 2]).all() and not ctx[:, Q // 2].any() and not got[0][:, Q // 2].any() and not dq[:, Q // 2].any()
    if kind == "key":         # an unseen key: zero dk, dv
        assert not got[1][:, HW // 2].any() and not got[2][:, HW // 2].any() and not dk[:, HW // 2].any()


def test_oracle_is_multihead_attention():
    """The plain sequence of the oracle is nn.MultiheadAttention's core: same output under a per-head boolean mask, fp64."""
    Fr, heads, C, Q, HW = 2, 2, 16, 5, 9
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(C, heads).double()
    x, y = torch.randn(Q, Fr, C, dtype=torch.float64), torch.randn(HW, Fr, C, dtype=torch.float64)
    m = torch.rand(Fr, heads, Q, HW) < 0.5
    m[..., 0] = False
    want = mha(x, y, y, attn_mask=m.reshape(Fr * heads, Q, HW))[0].detach()
    w, b = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    lin = lambda t, i: torch.nn.functional.linear(t.transpose(0, 1), w[i * C:(i + 1) * C], b[i * C:(i + 1) * C])      # noqa: E731
    ctx, _ = MO.attention(lin(x, 0), lin(y, 1), lin(y, 2), m, heads)
    got = mha.out_proj(ctx).transpose(0, 1).detach()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_parameter_tree_and_state_dict():
    ma = _ma()
    for bias in (True, False):
        torch.manual_seed(5)
        ref = nn.MultiheadAttention(64, 4, bias=bias)
        torch.manual_seed(5)
        mod = ma.MaskedMultiheadAttention(64, 4, bias=bias)
        a, b = dict(ref.named_parameters()), dict(mod.named_parameters())
        assert list(a) == list(b)
        for n in a:
            assert a[n].shape == b[n].shape and torch.equal(a[n], b[n]), n      # the same initialisation from the same seed
        assert list(ref.state_dict()) == list(mod.state_dict())
        torch.manual_seed(6)
        other = nn.MultiheadAttention(64, 4, bias=bias)
        mod.load_state_dict(other.state_dict(), strict=True)
        ref.load_state_dict(mod.state_dict(), strict=True)
        for n, p in other.named_parameters():
            assert torch.equal(p, dict(mod.named_parameters())[n]) and torch.equal(p, dict(ref.named_parameters())[n])


def test_use_native_attention_shares_parameters():
    ma = _ma()

    class Layer(nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn = nn.MultiheadAttention(32, 4)
            self.inner = nn.ModuleList([nn.MultiheadAttention(32, 2, dropout=0.0), nn.Linear(4, 4)])
            self.wide = nn.MultiheadAttention(32, 4, kdim=16, vdim=16)          # not compatible: stays
            self.first = nn.MultiheadAttention(32, 4, batch_first=True)         # not compatible: stays

    net = Layer()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    params = {n: p for n, p in net.named_parameters()}
    assert ma.use_native_attention(net) == 2
    assert isinstance(net.self_attn, ma.MaskedMultiheadAttention) and isinstance(net.inner[0], ma.MaskedMultiheadAttention)
    assert type(net.wide) is nn.MultiheadAttention and type(net.first) is nn.MultiheadAttention
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p is params[n] for n, p in net.named_parameters())
    assert ma.use_native_attention(net) == 0


def test_refusals():
    ma = _ma()
    with pytest.raises(NotImplementedError, match="batch_first"):
        ma.MaskedMultiheadAttention(32, 4, batch_first=True)
    with pytest.raises(NotImplementedError, match="kdim"):
        ma.MaskedMultiheadAttention(32, 4, kdim=16)
    with pytest.raises(NotImplementedError, match="kdim"):
        ma.MaskedMultiheadAttention(32, 4, vdim=16)
    with pytest.raises(ValueError, match="head width"):
        ma.MaskedMultiheadAttention(48, 4)
    mod = ma.MaskedMultiheadAttention(32, 4)
    x, y = torch.randn(3, 2, 32), torch.randn(5, 2, 32)
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        mod(x, y, y, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="need_weights"):
        mod(x, y, y, need_weights=True)
    with pytest.raises(TypeError, match="float masks"):
        mod(x, y, y, attn_mask=torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(x, y, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(x, y, y, attn_mask=torch.zeros(3, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ma.masked_attention(x.transpose(0, 1), y.transpose(0, 1), y.transpose(0, 1), None, heads=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ma.pack_attention_mask(torch.zeros(2, 3, 5, dtype=torch.bool))
    with pytest.raises(TypeError, match="float masks"):
        ma.pack_attention_mask(torch.zeros(2, 3, 5))
    wet = ma.MaskedMultiheadAttention(32, 4, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        wet(x, y, y)
    wet.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # dropout is no obstacle in eval mode: the next refusal is the device
        wet(x, y, y)
    if torch.cuda.is_available():                                   # the mask is looked at once the tensors are on the GPU
        dev = torch.device("cuda:0")
        mod, x, y = mod.to(dev), x.to(dev), y.to(dev)
        with pytest.raises(TypeError, match="float masks"):
            mod(x, y, y, attn_mask=torch.zeros(3, 5, device=dev))
        with pytest.raises(ValueError, match="attn_mask"):
            mod(x, y, y, attn_mask=torch.zeros(4, 3, 5, dtype=torch.bool, device=dev))


def test_pack_agrees_with_oracle():
    """pack_attention_mask against tests/mask_decoder_oracle.pack_mask where it can run: the oracle packs the mask with its padding
    keys hidden, the layout with the padding bits set."""
    if not torch.cuda.is_available():
        pytest.skip("pack_attention_mask runs on the GPU (tests/test_masked_attention.py covers it there)")
    ma = _ma()
    rs = np.random.RandomState(2)
    for HW in (1, 31, 32, 33, 100):
        m = rs.random_sample((2, 3, HW)) < 0.5
        padded = np.concatenate([m, np.ones((2, 3, (-HW) % 32), bool)], -1)
        got = ma.pack_attention_mask(torch.from_numpy(m).to("cuda:0"))
        assert got.HW == HW and not got.per_head
        assert np.array_equal(got.words.cpu().numpy(), DO.pack_mask(padded))
