"""Helper of the text-tower tests (not a test file): the SigLIP text tower restated in torch from the model's definition, with a
key-padding mask, at a chosen precision.  Nothing here imports ``transformers`` or the package under test.

    x        = token_embedding[ids] + position_embedding[arange(L)]
    layer    : x += out_proj(attention(qkv(LN1(x)), key_mask));  x += fc2(act(fc1(LN2(x))))          (pre-LN)
    last     = final_layer_norm(x);  pooled = head(last[:, L - 1])                                  (the last position, masked or not)
    attention: softmax(q k^T / sqrt(head_dim) + (0 | -inf)[key]) v  per (caption, head), non-causal

``forward(..., dtype=torch.float64)`` is the reference; ``dtype=torch.float32`` and ``bf16_operands=True`` are the two precision
floors of the GPU tests: the same operator sequence at the operand precision of the accurate mode (fp32) and of the bf16 mode (both
operands of the four Linears of a layer rounded to bf16, products accumulated in fp32; everything else, the pooled head included, fp32).
``bf16_operands="x3"`` is the accurate mode's own operand precision: hi + lo bf16 planes of both operands, three of the four products.

The fixture ``tests/golden/f18_text_tower.npz`` holds ids, masks and the outputs of HF ``SiglipTextModel``, not the weights: the wider
configuration alone has 2.9 M of them (12 MB), so the fixture records the seed and ``make_weights`` redraws them — from
``numpy.random.RandomState``, whose streams are frozen across NumPy versions — in the generator (``tools/make_golden_text_tower.py``)
and in the tests alike.
"""
import math
import os

import numpy as np
import torch

from tests.oracle_ops import activation, layernorm, operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f18_text_tower.npz")

CONFIGS = {
    "d128": dict(vocab_size=97, max_position_embeddings=16, hidden_size=128, num_attention_heads=2, intermediate_size=256,
                 num_hidden_layers=2, projection_size=128, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6),
    "hd72": dict(vocab_size=97, max_position_embeddings=16, hidden_size=576, num_attention_heads=8, intermediate_size=1072,
                 num_hidden_layers=1, projection_size=576, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6),
}
SEEDS = {"d128": 1801, "hd72": 1802}


def weight_shapes(cfg):
    D, I, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_size"]
    out = {"embeddings.token_embedding.weight": (cfg["vocab_size"], D),
           "embeddings.position_embedding.weight": (cfg["max_position_embeddings"], D)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            out[p + ln + ".weight"] = (D,)
            out[p + ln + ".bias"] = (D,)
        for a in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[p + f"self_attn.{a}.weight"] = (D, D)
            out[p + f"self_attn.{a}.bias"] = (D,)
        out[p + "mlp.fc1.weight"] = (I, D)
        out[p + "mlp.fc1.bias"] = (I,)
        out[p + "mlp.fc2.weight"] = (D, I)
        out[p + "mlp.fc2.bias"] = (D,)
    out["final_layer_norm.weight"] = (D,)
    out["final_layer_norm.bias"] = (D,)
    out["head.weight"] = (P, D)
    out["head.bias"] = (P,)
    return out


def make_weights(cfg, seed):
    """fp32 state dict under HF's key names: matrices N(0, 1 / fan_in), embeddings N(0, 0.5^2), biases N(0, 0.1^2), LayerNorm
    gamma 1 + N(0, 0.1^2) and beta N(0, 0.1^2) — a unit-scale residual stream with attention that is neither flat nor one-hot."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shape in weight_shapes(cfg).items():
        z = rs.standard_normal(shape)
        if "embedding" in k:
            v = 0.5 * z
        elif "layer_norm" in k:
            v = (1.0 if k.endswith(".weight") else 0.0) + 0.1 * z
        elif k.endswith(".bias"):
            v = 0.1 * z
        else:
            v = z / math.sqrt(shape[1])
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def make_ids_and_masks(cfg, seed, B=3):
    """ids [3, L]; ``mask`` with valid lengths L, 5 and 1 (right-padded); ``mask_last`` with the LAST position masked."""
    L = cfg["max_position_embeddings"]
    rs = np.random.RandomState(seed + 7)
    ids = rs.randint(0, cfg["vocab_size"], size=(B, L)).astype(np.int64)
    mask = np.zeros((B, L), dtype=np.int64)
    for b, n in enumerate((L, 5, 1)):
        mask[b, :n] = 1
    mask_last = np.ones((B, L), dtype=np.int64)
    mask_last[:, L - 1] = 0
    return torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(mask_last)


def attention(qkv, mask, heads):
    """qkv [B, L, 3D] (q | k | v columns), mask [B, L] (0 = masked key) or None -> [B, L, D], in qkv's dtype."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, L, heads, hd).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, L, D)


def pool(x, gamma, beta, eps, w, b, group=0):
    """x [B, L, D] -> head(LN(x[:, L - 1])) [B, P]; group >= 1: normalise rows, mean over ``group`` consecutive rows, normalise."""
    row = x[:, -1]
    if gamma is not None:
        row = layernorm(row, gamma, beta, eps)
    out = row @ w.t() + (b if b is not None else 0.0)
    if group:
        out = out / out.norm(dim=-1, keepdim=True)
        out = out.reshape(-1, group, out.shape[-1]).mean(dim=1)
        out = out / out.norm(dim=-1, keepdim=True)
    return out


def forward(sd, cfg, ids, mask=None, dtype=torch.float64, bf16_operands=False):
    """(last_hidden_state [B, L, D], pooler_output [B, P]) in ``dtype``."""
    W = {k: v.to(dtype) for k, v in sd.items()}
    eps, act, heads = cfg["layer_norm_eps"], cfg["hidden_act"], cfg["num_attention_heads"]
    L = ids.shape[1]
    x = W["embeddings.token_embedding.weight"][ids] + W["embeddings.position_embedding.weight"][:L][None]
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        h = layernorm(x, W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], eps)
        wqkv = torch.cat([W[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0)
        bqkv = torch.cat([W[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], dim=0)
        ctx = attention(operand_linear(h, wqkv, bqkv, bf16_operands), mask, heads)
        x = x + operand_linear(ctx, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"], bf16_operands)
        h = layernorm(x, W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], eps)
        h = activation(operand_linear(h, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"], bf16_operands), act)
        x = x + operand_linear(h, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"], bf16_operands)
    last = layernorm(x, W["final_layer_norm.weight"], W["final_layer_norm.bias"], eps)
    return last, last[:, -1] @ W["head.weight"].t() + W["head.bias"]


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_case(gold, name, which):
    """which in ("nomask", "mask", "mask_last") -> (mask tensor or None, last_hidden_state, pooler_output) of the fixture."""
    mask = None if which == "nomask" else torch.from_numpy(gold[f"{name}.{which}"])
    return mask, torch.from_numpy(gold[f"{name}.{which}.last_hidden_state"]), torch.from_numpy(gold[f"{name}.{which}.pooler_output"])
