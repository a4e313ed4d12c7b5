"""Helper of the online-action-detection tests (not a test file): the reference's LSTRStream.stream_inference path restated in torch at
a chosen precision, written out explicitly.  Nothing here imports the package under test or the reference.

    feature head   ReLU(LN(Linear(x)))  (identity when LINEAR_ENABLED is False), one head for long samples and one for work frames
    long memory    a ring of L projected rows per stream: k = W_k x, v = W_v x WITHOUT bias; window position i (0 = oldest) adds
                   k_pos[i] = W_k pe[i] + b_k, v_pos[i] = W_v pe[i] + b_v
    stage 0        tgt0 = norm1(queries + self_attn(queries)), q0 = W_q tgt0 + b_q  (input independent)
                   scores = head_dim^-0.5 q0 (k + k_pos)^T + key_mask;  ctx = softmax(scores) (v + v_pos)
                   x = norm2(tgt0 + out_proj(ctx)); x = norm3(x + FFN(x)); module norm.  Cached: a step without a long sample reuses it
    later stages   decoder layers over queries, or encoder layers, plain attention
    work memory    feature head + pe[L : L + W]; decoder layers (causal self-attention, cross-attention to the compressed memory, FFN),
                   all post-LN; classifier

``Stream(..., dtype=torch.float64)`` is the reference; ``dtype=torch.float32`` with ``bf16_operands="x3"`` / ``True`` are the precision
floors of the GPU tests (tests/oracle_ops.py: both operands of every Linear as hi + lo bf16 planes, three of four products /
rounded to bf16; everything else in fp32).  ``from_scratch`` evaluates one step from a whole window, without a ring.
"""
import math
import os

import numpy as np
import torch

from tests.oracle_ops import activation, layernorm, operand_linear

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f20_oad.npz")
LN_EPS = 1e-5

CASES = {
    "a": dict(d_in=64, d_model=128, heads=4, ffn=192, activation="gelu", enc_module=[[4, 1, True], [-1, 1, True]], dec_module=[-1, 2, True],
              long_samples=12, work_samples=6, classes=7, linear_enabled=True),
    "b": dict(d_in=128, d_model=128, heads=2, ffn=192, activation="relu", enc_module=[[4, 1, False], [3, 1, True]], dec_module=[-1, 2, True],
              long_samples=8, work_samples=5, classes=7, linear_enabled=False),
}
FULL = dict(d_in=768, d_model=1024, heads=4, ffn=1024, activation="relu", enc_module=[[16, 1, True], [32, 2, True]], dec_module=[-1, 2, True],
            long_samples=64, work_samples=32, classes=22, linear_enabled=True)


def positional_table(rows, d):
    """The reference's sinusoid table, computed in fp32 as it does (position_encoding.py)."""
    pe = torch.zeros(rows, d)
    position = torch.arange(0, rows, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2).float() * (-math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def weight_shapes(cfg):
    d, F, din = cfg["d_model"], cfg["ffn"], cfg["d_in"]
    out = {}

    def layer(p, decoder):
        for a in (("self_attn", "multihead_attn") if decoder else ("self_attn",)):
            out[f"{p}{a}.in_proj_weight"] = (3 * d, d)
            out[f"{p}{a}.in_proj_bias"] = (3 * d,)
            out[f"{p}{a}.out_proj.weight"] = (d, d)
            out[f"{p}{a}.out_proj.bias"] = (d,)
        out[p + "linear1.weight"] = (F, d)
        out[p + "linear1.bias"] = (F,)
        out[p + "linear2.weight"] = (d, F)
        out[p + "linear2.bias"] = (d,)
        for n in (("norm1", "norm2", "norm3") if decoder else ("norm1", "norm2")):
            out[f"{p}{n}.weight"] = (d,)
            out[f"{p}{n}.bias"] = (d,)

    if cfg["linear_enabled"]:
        for fh in ("feature_head_long", "feature_head_work"):
            out[fh + ".visual_linear.0.weight"] = (d, din)
            out[fh + ".visual_linear.0.bias"] = (d,)
            out[fh + ".visual_linear.1.weight"] = (d,)
            out[fh + ".visual_linear.1.bias"] = (d,)
    for j, (q, layers, norm) in enumerate(cfg["enc_module"]):
        if q != -1:
            out[f"enc_queries.{j}.weight"] = (q, d)
        for i in range(layers):
            layer(f"enc_modules.{j}.layers.{i}.", q != -1)
        if norm:
            out[f"enc_modules.{j}.norm.weight"] = (d,)
            out[f"enc_modules.{j}.norm.bias"] = (d,)
    for i in range(cfg["dec_module"][1]):
        layer(f"dec_modules.layers.{i}.", True)
    if cfg["dec_module"][2]:
        out["dec_modules.norm.weight"] = (d,)
        out["dec_modules.norm.bias"] = (d,)
    out["classifier.weight"] = (cfg["classes"], d)
    out["classifier.bias"] = (cfg["classes"],)
    return out


def make_weights(cfg, seed):
    """fp32 state dict under the reference's names: matrices N(0, 1 / fan_in), queries N(0, 1), biases N(0, 0.1^2), LayerNorm gamma
    1 + N(0, 0.1^2), beta N(0, 0.1^2); numpy.random.RandomState streams are frozen across NumPy versions."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shape in weight_shapes(cfg).items():
        z = rs.standard_normal(shape)
        if k.startswith("enc_queries"):
            v = z
        elif "norm" in k or ".visual_linear.1." in k:
            v = (1.0 if k.endswith("weight") else 0.0) + 0.1 * z
        elif k.endswith("bias"):
            v = 0.1 * z
        else:
            v = z / math.sqrt(shape[1])
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def _ln(x, g, b):
    return layernorm(x, g, b, LN_EPS)


def attention(q, k, v, heads, mask=None, causal=False):
    """q [Tq, D], k / v [Tk, D], mask additive [Tk] or None -> [Tq, D]; causal: key j visible to query i iff j <= i + Tk - Tq."""
    Tq, D = q.shape
    Tk = k.shape[0]
    hd = D // heads
    qh, kh, vh = (t.reshape(-1, heads, hd).permute(1, 0, 2) for t in (q, k, v))
    s = (qh * float(hd) ** -0.5) @ kh.transpose(1, 2)
    if mask is not None:
        s = s + mask.to(s.dtype)[None, None, :]
    if causal:
        i = torch.arange(Tq)[:, None]
        j = torch.arange(Tk)[None, :]
        s = s.masked_fill((j > i + (Tk - Tq))[None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).permute(1, 0, 2).reshape(Tq, D)


class Stream:
    """One stream of the detector.  ``step(work [W, d_in], long=None | [1, d_in] | [L, d_in], mask=None | [L])`` -> scores [W, C]."""

    def __init__(self, sd, cfg, dtype=torch.float64, bf16_operands=False):
        self.cfg, self.dtype, self.bo = cfg, dtype, bf16_operands
        self.W = {k: v.to(dtype) for k, v in sd.items() if k != "pos_encoding.pe"}
        self.d, self.L, self.heads = cfg["d_model"], cfg["long_samples"], cfg["heads"]
        self.pe = positional_table(self.L + cfg["work_samples"], self.d).to(dtype)
        if cfg["enc_module"][0][0] == -1 or cfg["enc_module"][0][1] != 1:
            raise RuntimeError("stage 0 of the stream path is one decoder layer over queries")
        d, p = self.d, "enc_modules.0.layers.0."
        w, b = self.W[p + "multihead_attn.in_proj_weight"], self.W[p + "multihead_attn.in_proj_bias"]
        self.w_kv, self.b_kv = w[d:], b[d:]
        # input independent: the queries' self-attention + norm1, their q projection, the positional addends
        tgt = self.W["enc_queries.0.weight"]
        self.tgt0 = self._self_attn(p, tgt, False)
        self.q0 = operand_linear(self.tgt0, w[:d], b[:d], self.bo)
        self.pos_kv = operand_linear(self.pe[:self.L], self.w_kv, self.b_kv, self.bo)
        self.ring = torch.zeros(self.L, 2 * d, dtype=dtype)      # W_k x | W_v x by SLOT
        self.head = 0                                             # slot of the oldest sample
        self.fill = 0
        self.mem0 = None

    # ---- sublayers -------------------------------------------------------------------------------------------------------------
    def _feature_head(self, which, x):
        x = x.to(self.dtype)
        if not self.cfg["linear_enabled"]:
            return x
        p = f"feature_head_{which}.visual_linear."
        return torch.relu(_ln(operand_linear(x, self.W[p + "0.weight"], self.W[p + "0.bias"], self.bo), self.W[p + "1.weight"], self.W[p + "1.bias"]))

    def _self_attn(self, p, x, causal):
        d = self.d
        qkv = operand_linear(x, self.W[p + "self_attn.in_proj_weight"], self.W[p + "self_attn.in_proj_bias"], self.bo)
        ctx = attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], self.heads, causal=causal)
        y = operand_linear(ctx, self.W[p + "self_attn.out_proj.weight"], self.W[p + "self_attn.out_proj.bias"], self.bo)
        return _ln(x + y, self.W[p + "norm1.weight"], self.W[p + "norm1.bias"])

    def _cross_attn(self, p, x, mem):
        d = self.d
        w, b = self.W[p + "multihead_attn.in_proj_weight"], self.W[p + "multihead_attn.in_proj_bias"]
        q = operand_linear(x, w[:d], b[:d], self.bo)
        kv = operand_linear(mem, w[d:], b[d:], self.bo)
        y = operand_linear(attention(q, kv[:, :d], kv[:, d:], self.heads), self.W[p + "multihead_attn.out_proj.weight"],
                    self.W[p + "multihead_attn.out_proj.bias"], self.bo)
        return _ln(x + y, self.W[p + "norm2.weight"], self.W[p + "norm2.bias"])

    def _ffn(self, p, x, norm):
        h = activation(operand_linear(x, self.W[p + "linear1.weight"], self.W[p + "linear1.bias"], self.bo), self.cfg["activation"])
        y = operand_linear(h, self.W[p + "linear2.weight"], self.W[p + "linear2.bias"], self.bo)
        return _ln(x + y, self.W[p + norm + ".weight"], self.W[p + norm + ".bias"])

    def _module_norm(self, p, x, on):
        return _ln(x, self.W[p + "norm.weight"], self.W[p + "norm.bias"]) if on else x

    # ---- the stages ------------------------------------------------------------------------------------------------------------
    def _stage0(self, kv_window, mask):
        """kv_window [L, 2d]: W_k x | W_v x, oldest first."""
        d, p = self.d, "enc_modules.0.layers.0."
        kv = kv_window + self.pos_kv
        ctx = attention(self.q0, kv[:, :d], kv[:, d:], self.heads, mask=mask)
        y = operand_linear(ctx, self.W[p + "multihead_attn.out_proj.weight"], self.W[p + "multihead_attn.out_proj.bias"], self.bo)
        x = _ln(self.tgt0 + y, self.W[p + "norm2.weight"], self.W[p + "norm2.bias"])
        x = self._ffn(p, x, "norm3")
        return self._module_norm("enc_modules.0.", x, self.cfg["enc_module"][0][2])

    def _tail(self, mem, work):
        cfg = self.cfg
        for j, (q, layers, norm) in enumerate(cfg["enc_module"]):
            if j == 0:
                continue
            m = f"enc_modules.{j}."
            if q != -1:
                x = self.W[f"enc_queries.{j}.weight"]
                for i in range(layers):
                    p = f"{m}layers.{i}."
                    x = self._ffn(p, self._cross_attn(p, self._self_attn(p, x, False), mem), "norm3")
                mem = x
            else:
                for i in range(layers):
                    p = f"{m}layers.{i}."
                    mem = self._ffn(p, self._self_attn(p, mem, False), "norm2")
            mem = self._module_norm(m, mem, norm)
        x = self._feature_head("work", work) + self.pe[self.L:self.L + work.shape[0]]      # padding = long_memory_num_samples
        for i in range(cfg["dec_module"][1]):
            p = f"dec_modules.layers.{i}."
            x = self._ffn(p, self._cross_attn(p, self._self_attn(p, x, True), mem), "norm3")
        x = self._module_norm("dec_modules.", x, cfg["dec_module"][2])
        return operand_linear(x, self.W["classifier.weight"], self.W["classifier.bias"], self.bo)

    def step(self, work, long=None, mask=None):
        L = self.L
        if long is not None:
            rows = operand_linear(self._feature_head("long", long), self.w_kv, None, self.bo)
            if rows.shape[0] == L and self.fill == 0:
                self.ring[:] = rows
                self.head, self.fill = 0, L
            elif rows.shape[0] == 1 and self.fill == L:
                self.ring[self.head] = rows[0]                     # over the oldest
                self.head = (self.head + 1) % L
            else:
                raise ValueError("an empty stream takes the whole window, a filled one a single sample")
            window = torch.cat([self.ring[self.head:], self.ring[:self.head]])      # oldest first
            self.mem0 = self._stage0(window, mask)
        if self.mem0 is None:
            raise ValueError("the first step needs the long window")
        return self._tail(self.mem0, work)

    def from_scratch(self, work, window, mask=None):
        """The same step computed from the whole window of raw long samples [L, d_in] (oldest first), no ring, no cache."""
        kv = operand_linear(self._feature_head("long", window), self.w_kv, None, self.bo)
        return self._tail(self._stage0(kv, mask), work)


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_case(gold, name):
    """-> (state dict fp32 without pe, redrawn from the stored seed; steps) with steps = list of (work [W, d_in], long or None,
    mask or None, scores [W, C])."""
    sd = make_weights(CASES[name], int(gold[f"{name}.seed"]))
    work, longs, first = gold[f"{name}.work"], gold[f"{name}.long"], gold[f"{name}.long_window"]
    masks, scores, has_long = gold[f"{name}.mask"], gold[f"{name}.scores"], gold[f"{name}.has_long"]
    steps = []
    for t in range(work.shape[0]):
        if t == 0:
            lg = torch.from_numpy(first)
        else:
            lg = torch.from_numpy(longs[t:t + 1]) if has_long[t] else None
        mk = torch.from_numpy(masks[t]) if has_long[t] else None
        steps.append((torch.from_numpy(work[t]), lg, mk, torch.from_numpy(scores[t])))
    return sd, steps


def state_dict_keys(gold, name):
    return [str(k) for k in gold[f"{name}.keys"]]
