"""Helper of tests/test_backward_precision.py (not a test file): the single backward operators of the training step restated in plain torch
at a chosen precision.  Nothing here imports the package under test.

    attention_forward(qkv, heads, hd, causal)                 fp64 context O = softmax(scale Q K^T [+ causal mask]) V
    attention_backward(qkv, o, d_o, heads, hd, causal, ...)   d_qkv of the same attention, written out (no autograd), in fp64 or fp32:
        mode "exact"    no rounding anywhere; Delta = rowsum(P o dP), i.e. what autograd gives (`o` is not read)
        mode "tuned"    a bf16 rounding wherever the head_dim-64 kernels (csrc/sf_attention_bwd.hip) make one:
                          Delta_i = sum_e dO_ie O_ie from the bf16 `o` that the forward stored   (stage_problem)
                          P rounded to bf16 as the A operand of dV = P^T dO                      (pack_a(p..) in phase B)
                          dS = P o (dP - Delta) * scale from the UNROUNDED P, rounded to bf16 as the A operand of
                          dQ = dS K and dK = dS^T Q                                             (pack_a(ds..) in phases B and C)
                          the three results rounded to bf16                                      (store_patch)
        mode "generic"  the generic-width kernel (csrc/sf_attention_generic_bwd.hip): fp32 throughout from the bf16 operands and the
                        bf16 `o`; only the three results are rounded
        fault           a deliberately wrong dS, for the check that the metrics can fail: "ds_scale" (dS * 1.01), "drop_last_query"
                        (dS of the last query row zeroed), "half_last_key" (dS column of the last key halved)
    layernorm_backward(x, dy, gamma, g_in, eps, dtype)        autograd of torch.nn.functional.layer_norm: (g_in + dx, d_gamma, d_beta)
    wgrad(dy, x, dtype)                                       dy^T x

Sequences are [nseq, L, C] here; to_sequences / from_sequences convert the temporal token order (row of (b, t, n) = (b*L + t)*N + n).
"""
import torch
import torch.nn.functional as F

from tests.oracle_ops import bf16_round

FAULTS = ("ds_scale", "drop_last_query", "half_last_key")


def to_sequences(x):
    """[B, L, N, C] (temporal token order) -> [B*N, L, C]"""
    B, L, N, C = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, L, C)


def from_sequences(x, B, N):
    """[B*N, L, C] -> [B, L, N, C]"""
    _, L, C = x.shape
    return x.reshape(B, N, L, C).permute(0, 2, 1, 3).contiguous()


def _split(t, heads, hd, dtype):
    nseq, L, _ = t.shape
    return t.to(dtype).reshape(nseq, L, -1, heads, hd).permute(2, 0, 3, 1, 4)      # [parts, nseq, heads, L, hd]


def _merge(t):
    nseq, heads, L, hd = t.shape
    return t.transpose(1, 2).reshape(nseq, L, heads * hd)


def _probabilities(q, k, hd, causal, pos=None):
    L = q.shape[-2]
    s = q @ k.transpose(-1, -2) * (hd ** -0.5)
    if causal:
        pos = torch.arange(L) if pos is None else pos          # query at position pos[i] sees the keys at positions <= pos[i]
        s = s.masked_fill(pos[:, None] < pos[None, :], float("-inf"))
    return s.softmax(-1)


def attention_forward(qkv, heads, hd, causal):
    q, k, v = _split(qkv, heads, hd, torch.float64)
    return _merge(_probabilities(q, k, hd, causal) @ v)


def attention_backward(qkv, o, d_o, heads, hd, causal, dtype=torch.float64, mode="exact", fault=None, order=None):
    """order: None, or an integer that draws another SUMMATION ORDER of the same operator on the same inputs — one permutation of the
    head_dim columns (the contraction of S, dP and Delta) and one of the token positions (the contraction of dQ, dK, dV and of the row
    sums; the causal mask follows the positions), undone on the result.  Exact arithmetic does not see it; fp32 rounds differently."""
    assert mode in ("exact", "tuned", "generic") and fault in (None,) + FAULTS
    q, k, v = _split(qkv, heads, hd, dtype)
    g = _split(d_o, heads, hd, dtype)[0]
    oo = _split(o, heads, hd, dtype)[0]
    L = q.shape[-2]
    pos = None
    if order is not None:
        assert fault is None
        gen = torch.Generator().manual_seed(7919 * order + L)
        cols, pos = torch.randperm(hd, generator=gen), torch.randperm(L, generator=gen)
        q, k, v, g, oo = (t[..., pos, :][..., cols].contiguous() for t in (q, k, v, g, oo))
    scale = hd ** -0.5
    p = _probabilities(q, k, hd, causal, pos)
    dp = g @ v.transpose(-1, -2)
    if mode == "exact":
        delta = (p * dp).sum(-1, keepdim=True)
    else:
        delta = (g * oo).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    if fault == "ds_scale":
        ds = ds * 1.01
    elif fault == "drop_last_query":
        ds = ds.clone()
        ds[..., -1, :] = 0
    elif fault == "half_last_key":
        ds = ds.clone()
        ds[..., :, -1] *= 0.5
    if mode == "tuned":
        p, ds = bf16_round(p), bf16_round(ds)
    parts = [ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g]
    if order is not None:
        inv_c, inv_p = torch.argsort(cols), torch.argsort(pos)
        parts = [t[..., inv_c][..., inv_p, :] for t in parts]
    out = torch.cat([_merge(t) for t in parts], dim=-1)
    return out if mode == "exact" else bf16_round(out)


def layernorm_backward(x, dy, gamma, g_in, eps, dtype=torch.float64):
    D = x.shape[-1]
    xr = x.to(dtype).requires_grad_(True)
    gr = gamma.to(dtype).requires_grad_(True)
    br = torch.zeros(D, dtype=dtype, requires_grad=True)
    F.layer_norm(xr, (D,), gr, br, eps).backward(dy.to(dtype))
    dx = xr.grad if g_in is None else xr.grad + g_in.to(dtype)
    return dx, gr.grad, br.grad


def wgrad(dy, x, dtype=torch.float64):
    return dy.to(dtype).t() @ x.to(dtype)


# ---------------------------------------------------------------------------------------------------
# metrics: the oracles import nothing that loads the library, so these stay beside tests.helpers' (whose guard is 1e-30, on CPU copies)
# ---------------------------------------------------------------------------------------------------
def rel_l2(got, want):
    got, want = got.double(), want.double()
    return float((got - want).norm() / (want.norm() + 1e-300))


def worst_row(got, want, heads, hd):
    """largest L2 error of one token row of one head over the root-mean-square row norm of the slice; [nseq, L, heads*hd] slices"""
    got, want = got.double().reshape(-1, heads, hd), want.double().reshape(-1, heads, hd)
    rms = float(want.norm(dim=-1).pow(2).mean().sqrt())
    return float((got - want).norm(dim=-1).max()) / (rms + 1e-300)


def rel_max(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))
