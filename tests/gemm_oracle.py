"""Oracle of ONE forward GEMM with its fused epilogue (not a test file): everything a kernel of csrc/sf_gemm*.hip writes for one
``SfGemmArgs``, in plain torch, from the operand planes the kernel reads.  Nothing here imports the package under test.

Like tests/oracle_ops.py every function works in the dtype it is asked for: ``reference(case, torch.float64)`` is the reference,
``reference(case, torch.float32)`` the FLOOR MODEL — the same expression in fp32 with the kernel's documented formula where it has one
(the fold epilogue ``rstd (acc - mean ln_s[n]) + b'``, ``gelu_bf16`` / ``gelu_fast`` / ``gelu_tanh`` restated from csrc/sf_common.h, the
statistics as sums of x and x^2).  What the floor model loses against fp64 is what a correct kernel may lose (tests/helpers.py,
``check_against_floor``).

A case is a ``Case``: planes are tensors whose VALUES are exact bf16 numbers (any float dtype); the test turns them into bit patterns.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

from tests.oracle_ops import activation, bf16_round, layernorm, operand_linear      # noqa: F401  (layernorm / operand_linear: re-exported)

F32, BF16, ACT_BF16, RESID_F32, EMBED_F32 = range(5)
ACT_NAMES = {0: "gelu", 1: "gelu_pytorch_tanh", 2: "relu"}
BF16_HALF_ULP = 2.0 ** -9          # half a bf16 ulp of v is at most 2^-9 |v|
TWO_PLANES_REL, THREE_PLANES_REL = 2.0 ** -17, 2.0 ** -25


# ---------------------------------------------------------------------------------------------------
# planes
# ---------------------------------------------------------------------------------------------------
def split_planes(v, n):
    """v as n bf16 planes, canonically: hi = bf16(v), lo = bf16(v - hi), lo2 = bf16(v - hi - lo); each in v's dtype."""
    out, rest = [], v
    for _ in range(n):
        p = bf16_round(rest)
        out.append(p)
        rest = rest - p
    return out


def is_nearest_bf16(hi, total):
    """hi is A nearest bf16 number to total (fp64, exact): bf16_round(total) itself, except that where total lies exactly half way between
    two bf16 numbers either of them is one.  (lo = bf16(v - hi) rounds up to exactly half an ulp of hi about once in 2^9 values, and
    round-to-nearest-even of hi + lo may then name the other neighbour: hi = bf16(v) is still right.)"""
    hi, total = hi.double(), total.double()
    return (total - hi).abs() <= (total - bf16_round(total)).abs()


def bf16_ulp(v):
    """The spacing of bf16 numbers at |v| (fp64): 2^(e - 7) for 2^e <= |v| < 2^(e + 1)."""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 7)


# ---------------------------------------------------------------------------------------------------
# the LayerNorm fold: operands of the consumer from (W, gamma, beta, b), as SfGemmArgs documents them
# ---------------------------------------------------------------------------------------------------
def fold_operands(W, gamma, beta, b, split):
    """W' = W gamma (fp32, then rounded to the planes the MFMAs read), ln_s[n] = sum_k of those planes, b' = b + W beta.
    Returns (planes of W' as fp64 tensors, ln_s fp32, b' fp32)."""
    Wd = W.double()
    wf = (Wd * gamma.double()).float()
    planes = [p.double() for p in split_planes(wf, 2 if split else 1)]
    ln_s = sum(planes).sum(dim=1).float()
    bp = ((b.double() if b is not None else 0.0) + Wd @ beta.double()).float()
    return planes, ln_s, bp


def fold_epilogue(acc, s1, s2, K, eps, ln_s, bias):
    """The consumer's epilogue from a row's sum x and sum x^2, as the kernels evaluate it."""
    mean = s1 / K
    var = (s2 / K - mean * mean).clamp_min(0.0) + eps
    rstd = 1.0 / torch.sqrt(var)
    y = rstd[:, None] * (acc - mean[:, None] * ln_s[None, :])
    return y if bias is None else y + bias


# ---------------------------------------------------------------------------------------------------
# statistics layouts: where the pairs {sum x, sum x^2} of a producer's new residual row go
# ---------------------------------------------------------------------------------------------------
def stats_layout(kind, N):
    """[(first float of the pair in the row, first column, one past the last column)], row width in floats.
        "panel"  : N = 768, rows of 8: pair 0 = columns 0..383, pair 2 = columns 384..767, pairs 1 and 3 stay zero
        "quarter": rows of 8, one pair per 192-column quarter (the tile family's statistics producers)
        "tile256": rows of 8, one pair per 256-column tile (the 256^2 kernel's plane producers), N <= 1024
    """
    if kind == "panel":
        assert N == 768
        return [(0, 0, 384), (4, 384, 768)], 8
    if kind == "quarter":
        assert N % 192 == 0 and N // 192 <= 4
        return [(2 * j, 192 * j, 192 * (j + 1)) for j in range(N // 192)], 8
    if kind == "tile256":
        assert N % 256 == 0 and N // 256 <= 4
        return [(2 * j, 256 * j, 256 * (j + 1)) for j in range(N // 256)], 8
    raise ValueError(kind)


def stats_rows(x, kind):
    """The statistics buffer [M, width] of rows x (in x's dtype), zeros where the layout writes nothing."""
    pairs, width = stats_layout(kind, x.shape[1])
    out = torch.zeros(x.shape[0], width, dtype=x.dtype)
    for at, c0, c1 in pairs:
        out[:, at] = _chunked_sum(x[:, c0:c1])
        out[:, at + 1] = _chunked_sum(x[:, c0:c1] * x[:, c0:c1])
    return out


def _chunked_sum(t):
    """Row sums the way the producers add them up: a lane's 8 consecutive columns first, then those partial sums one after the other in a
    fixed order (csrc/sf_gemm_tile.hip: "the CH chunk partials of a row summed in a fixed order").  In fp64 the order does not matter;
    in fp32 this is the floor of a sequential sum, which torch's pairwise ``sum`` would understate."""
    part = t.reshape(t.shape[0], -1, 8).sum(dim=2)
    s = part[:, 0].clone()
    for j in range(1, part.shape[1]):
        s = s + part[:, j]
    return s


def stats_totals(rows):
    """What a consumer makes of a statistics row: (sum x, sum x^2) over all its pairs."""
    return rows[:, 0::2].sum(dim=1), rows[:, 1::2].sum(dim=1)


# ---------------------------------------------------------------------------------------------------
# the row remap of the KV-cache appends
# ---------------------------------------------------------------------------------------------------
def out_rows(M, grp_rows=0, grp_stride=0, grp_off=0):
    """Output row of each m: m itself, or (m / grp_rows) * grp_stride + grp_off + m % grp_rows."""
    m = torch.arange(M)
    if grp_rows <= 0:
        return m
    return (m // grp_rows) * grp_stride + grp_off + m % grp_rows


# ---------------------------------------------------------------------------------------------------
# activations as the kernels evaluate them (csrc/sf_common.h)
# ---------------------------------------------------------------------------------------------------
def gelu_bf16(x):
    """sf_common.h gelu_bf16: max(x, 0) - |x| Phi(-|x|), Phi(-a) = 0.5 - a g(a^2), g a degree-7 polynomial, a clamped to 4."""
    a = x.abs().clamp_max(4.0)
    u = a * a
    r = u * -1.300031527e-09 + 1.057452934e-07
    for c in (-3.740224429e-06, 7.655379159e-05, -1.023336896e-03, 9.588709101e-03, -6.607423723e-02, 3.988095224e-01):
        r = r * u + c
    h = 0.5 - a * r
    return x.clamp_min(0.0) - x.abs() * h


def gelu_fast(x):
    """sf_common.h gelu_fast: x Phi(x) with Phi through Abramowitz-Stegun 7.1.26."""
    ax = x.abs()
    t = 1.0 / (0.2316418882 * ax + 1.0)
    poly = t * 0.5307027145 - 0.7265760135
    for c in (0.7107068705, -0.142248368, 0.127414796):
        poly = poly * t + c
    h = poly * t * torch.exp2(x * x * -0.72134752044)
    return x.clamp_min(0.0) - ax * h


def gelu_tanh(x):
    """sf_common.h gelu_tanh: 0.5 x (1 + tanh(k (x + 0.044715 x^3))), k = sqrt(2 / pi) as the kernel's constant, x^3 as x * x * x."""
    k = 0.7978845608028654
    return 0.5 * x * (1.0 + torch.tanh(k * (x + 0.044715 * x * x * x)))


def kernel_activation(v, act, how):
    """how: "exact" (the reference: the activation itself, oracle_ops.activation), otherwise the kernels' evaluation — "bf16" (bf16-mode
    epilogues: gelu_bf16), "fast" (256^2 kernel, accurate mode: gelu_fast), "ocml" (every other accurate-mode epilogue: erff);
    tanh-GELU is gelu_tanh and ReLU is max(x, 0) in every kernel."""
    if how == "exact":
        return activation(v, ACT_NAMES[act])
    if act == 2:
        return torch.relu(v)
    if act == 1:
        return gelu_tanh(v)
    if how == "bf16":
        return gelu_bf16(v)
    if how == "fast":
        return gelu_fast(v)
    return activation(v, "gelu")


# ---------------------------------------------------------------------------------------------------
# a case and its reference
# ---------------------------------------------------------------------------------------------------
@dataclass
class Case:
    a: list                                   # 1 (bf16 mode) or 2 (split) planes [M, K]
    w: list                                   # likewise [N, K]
    epi: int = F32
    bias: Optional[torch.Tensor] = None
    act: int = 0
    act_how: str = "bf16"                     # the floor model's activation (kernel_activation)
    alpha: float = 1.0
    resid: Optional[torch.Tensor] = None      # fp32 [M, N] ([resid_mod, N])
    resid_mod: int = 0
    resid_planes: Optional[list] = None       # 2 or 3 planes [M, N]
    out_planes: int = 1                       # bf16 outputs: planes written (1: hi only)
    pos: Optional[torch.Tensor] = None
    time_rows: Optional[torch.Tensor] = None
    grp: tuple = (0, 0, 0)
    stats_kind: Optional[str] = None          # producer: layout of ln_stats_out
    ln_stats: Optional[torch.Tensor] = None   # consumer: the statistics rows it is given (fp32)
    ln_s: Optional[torch.Tensor] = None
    ln_eps: float = 1e-6
    ln_inkernel: bool = False
    extra: dict = field(default_factory=dict)

    @property
    def split(self):
        return len(self.a) == 2

    @property
    def shape(self):
        return self.a[0].shape[0], self.w[0].shape[0], self.a[0].shape[1]


def accumulate(c, dtype):
    a, w = [p.to(dtype) for p in c.a], [p.to(dtype) for p in c.w]
    if c.split:      # small terms first, the hi * hi product last; the lo * lo product is dropped (oracle_ops.operand_linear "x3")
        return a[0] @ w[1].t() + a[1] @ w[0].t() + a[0] @ w[0].t()
    return a[0] @ w[0].t()


def reference(c, dtype):
    """Every output of the kernel for case c, computed in ``dtype``: {"value": the epilogue's result before it is stored,
    "stats": the statistics rows or None, "rows": the output row of each m}."""
    M, N, K = c.shape
    acc = accumulate(c, dtype)
    bias = None if c.bias is None else c.bias.to(dtype)
    if c.ln_s is not None:
        if c.ln_inkernel:
            x = sum(p.to(dtype) for p in c.a)
            s1, s2 = x.sum(dim=1), (x * x).sum(dim=1)
        else:
            s1, s2 = stats_totals(c.ln_stats.to(dtype))
        v = fold_epilogue(acc, s1, s2, K, c.ln_eps, c.ln_s.to(dtype), bias)
    else:
        v = acc if bias is None else acc + bias
    if c.epi == ACT_BF16:
        v = kernel_activation(v, c.act, "exact" if dtype == torch.float64 else c.act_how)
    elif c.epi == RESID_F32:
        if c.resid_planes is not None:
            r = sum(p.to(dtype) for p in c.resid_planes)
        else:
            r = c.resid.to(dtype)
            if c.resid_mod > 0:
                r = r[torch.arange(M) % c.resid_mod]
        v = r + c.alpha * v
    elif c.epi == EMBED_F32:
        m = torch.arange(M)
        Np, Tn = c.pos.shape[0], c.time_rows.shape[0]
        v = v + c.pos.to(dtype)[m % Np] + c.time_rows.to(dtype)[(m // Np) % Tn]
    stats = stats_rows(v, c.stats_kind) if c.stats_kind else None
    return {"value": v, "stats": stats, "rows": out_rows(M, *c.grp)}
