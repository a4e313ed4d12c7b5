"""Shared operators of the fp64 oracles (not a test file): the ONE statement of how the library's GEMMs round their operands, and the
rowwise operators every oracle restates.  Nothing here imports the package under test or the reference.

Every function works in the dtype of its arguments: fp64 gives the reference, fp32 with ``bf16_operands`` the precision floor of a compute
mode.  The evaluation order is part of the contract: the committed fixtures under tests/golden/ hold results of exactly these expressions.
"""
import math

import torch


def bf16_round(t):
    """t rounded to bf16 (round-to-nearest-even) and back, in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def operand_linear(x, w, b=None, bf16_operands=False):
    """x @ w.T (+ b) with the operands as one of the library's GEMM paths sees them; the accumulation stays in x's dtype.

        False    exact operands
        "x3"     the accurate mode: x = xh + xl, w = wh + wl (bf16 each); xh wh + xh wl + xl wh, the xl wl product dropped
        truthy   the bf16 mode: one bf16 rounding of x and of w
    """
    if bf16_operands == "x3":
        xh, wh = bf16_round(x), bf16_round(w)
        xl, wl = bf16_round(x - xh), bf16_round(w - wh)
        y = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    elif bf16_operands:
        y = bf16_round(x) @ bf16_round(w).t()
    else:
        y = x @ w.t()
    return y if b is None else y + b


def layernorm(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def activation(x, name):
    if name == "gelu_pytorch_tanh":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if name == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if name == "relu":
        return torch.relu(x)
    raise ValueError(name)
