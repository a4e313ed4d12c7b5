"""Shared by the training-step tests (not a test file): the trainer paired with oracle/train_oracle.py, the per-tensor gradient
comparison with its tolerances, and the torch-autograd reference of the attention backward.

Tolerances (bf16 MFMA operands, fp32 accumulation):
  single operators : max-abs error <= OP_TOL of the tensor's max-abs (inputs pre-rounded to bf16, so the only differences are the bf16
                     rounding of P/dS/outputs and summation order)
  whole-model grads: relative L2 error per tensor <= GRAD_REL_L2, cosine >= GRAD_COS vs the fp32 oracle; 0-dim parameters (temporal
                     gates, logit scale / bias) are single sums over ~1e6 bf16-rounded products with heavy cancellation: <= SCALAR_REL
"""
import os

import numpy as np
import torch

from tests.helpers import cosine, gpu_device, rel_l2

OP_TOL = 2e-2
GRAD_REL_L2 = 2.6e-2        # measured worst 1.7e-2 (head.probe, small model), 1.1e-2 on SigLIP-base; + 50 %
GRAD_COS = 0.9995           # measured lowest 0.99987
SCALAR_REL = 0.10           # measured worst 6.7e-2 (a temporal gate: one sum over ~1e6 bf16-rounded products)


def device():
    """cuda:0; skips without a GPU."""
    return gpu_device(or_skip=True)


def attn_ref(qkv, d_o, nseq, L, heads, hd, causal):
    """torch autograd reference on [nseq, L, 3D] fp64 tensors -> (o, d_qkv)."""
    D = heads * hd
    t = qkv.double().clone().requires_grad_(True)
    q, k, v = (t[..., i * D:(i + 1) * D].reshape(nseq, L, heads, hd).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(nseq, L, D)
    o.backward(d_o.double())
    return o.detach(), t.grad


def trainer_and_oracle(cfg, freeze, seed, lora, lr=1e-3, wd=0.05):
    from oracle import train_oracle as TO
    from streamformer_amd.init_weights import make_state_dict
    from streamformer_amd.training import StreamformerTrainer
    sd = make_state_dict(cfg, seed=seed, lora=lora)
    tr = StreamformerTrainer(cfg, sd, ["retrieval", "localization"], freeze_spatial=freeze, device=device(), lr=lr, weight_decay=wd)
    orc = TO.OracleTrainer(sd, cfg, ["retrieval", "localization"], freeze_spatial=freeze, lr=lr, weight_decay=wd)
    return tr, orc


def to_dev(ti, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in ti.items()}


def compare_grads(tr, orc, floor=1e-3, scalar_rel=SCALAR_REL):
    """rel-L2 and cosine per tensor against the oracle's autograd, 0-dim parameters against their family's median magnitude."""
    og = orc.grads()
    names = set(tr.parameter_names(trainable_only=True))
    assert names == set(og), sorted(names ^ set(og))[:6]
    gmax = max(float(v.abs().max()) for v in og.values())
    report = {}
    for n, want in og.items():
        got = tr.grad(n).detach().cpu()
        if float(want.abs().max()) < floor * gmax * 1e-3:        # gradient that is (numerically) zero: absolute check
            assert float((got - want).abs().max()) < floor * gmax, n
            continue
        report[n] = (rel_l2(got, want), cosine(got, want))
    scalars = {n: r for n, r in report.items() if og[n].numel() == 1}
    report = {n: r for n, r in report.items() if og[n].numel() > 1}
    if os.environ.get("SF_TEST_VERBOSE"):
        for n in scalars:
            print(f"[0-dim] {n}: got {float(tr.grad(n)):+.5e} want {float(og[n]):+.5e} rel {scalars[n][0]:.3e}")
    # 0-dim parameters: one sum over ~1e6 bf16-rounded products with heavy cancellation.  A gate whose gradient happens to cancel to
    # 1e-4 when its eleven siblings sit at 5e-2 carries the same ABSOLUTE error as they do, so the bound is relative to the
    # larger of the value and the family's median magnitude (family = last name component: the twelve temporal gates, ...)
    fam = {}
    for n in scalars:
        fam.setdefault(n.rsplit(".", 1)[-1], []).append(abs(float(og[n])))
    for n, r in scalars.items():
        w = float(og[n])
        scale = max(abs(w), float(np.median(fam[n.rsplit(".", 1)[-1]])))
        assert abs(float(tr.grad(n)) - w) < scalar_rel * scale, (n, r, float(tr.grad(n)), w, scale)
    worst = max(report.items(), key=lambda kv: kv[1][0])
    wc = min(report.items(), key=lambda kv: kv[1][1])
    ws = max(scalars.items(), key=lambda kv: kv[1][0]) if scalars else ("-", (0.0, 1.0))
    print(f"[grad parity] worst rel-L2 {worst[1][0]:.3e} ({worst[0]}), lowest cosine {wc[1][1]:.6f} ({wc[0]}), worst 0-dim rel {ws[1][0]:.3e} ({ws[0]})")
    assert worst[1][0] < GRAD_REL_L2, worst
    assert wc[1][1] > GRAD_COS, wc
    return report
