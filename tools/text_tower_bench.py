"""Time of the native SigLIP text tower against the same operator sequence in torch, on the same GPU, in the same process.

    python tools/text_tower_bench.py            # writes profiles/text_tower.txt

SigLIP-base text shapes (vocab 32000, D 768, 12 layers, 12 heads, I 3072, L 64), random weights:
  * per-step case: 8 captions per call, with the tokenizer's attention mask, both compute modes;
  * class-table case: 400 labels x 28 templates = 11200 prompts of 64 tokens through ``encode_groups`` in chunks of whole labels (the
    chunking of ``encode_label_prompts``), both compute modes.
HIP events around the calls, median of the timed repetitions.  The torch side runs ``torch.nn.functional`` ops on the same weights
(fp32, and bf16 weights / activations for the bf16 mode's neighbour), key-padding mask as an additive bias.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import streamformer_amd as sa  # noqa: E402
from streamformer_amd.text import PROMPTS_PER_CALL  # noqa: E402
from tools._timing import timed  # noqa: E402


def torch_tower(sd, cfg, ids, mask, dtype):
    W = {k: v.to(dtype) for k, v in sd.items()}
    B, L = ids.shape
    H, D = cfg.num_attention_heads, cfg.hidden_size
    x = W["embeddings.token_embedding.weight"][ids] + W["embeddings.position_embedding.weight"][:L]
    bias = None
    if mask is not None:
        bias = torch.zeros(B, 1, 1, L, dtype=dtype, device=ids.device).masked_fill((mask == 0)[:, None, None, :], float("-inf"))
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        h = F.layer_norm(x, (D,), W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], cfg.layer_norm_eps)
        q, k, v = (F.linear(h, W[p + f"self_attn.{n}_proj.weight"], W[p + f"self_attn.{n}_proj.bias"]).view(B, L, H, D // H).transpose(1, 2)
                   for n in "qkv")
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=bias).transpose(1, 2).reshape(B, L, D)
        x = x + F.linear(a, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (D,), W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], cfg.layer_norm_eps)
        h = F.gelu(F.linear(h, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"]), approximate="tanh")
        x = x + F.linear(h, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"])
    last = F.layer_norm(x, (D,), W["final_layer_norm.weight"], W["final_layer_norm.bias"], cfg.layer_norm_eps)
    return F.linear(last[:, -1], W["head.weight"], W["head.bias"])


def torch_table(sd, cfg, ids, G, dtype, per_call):
    rows = []
    for i in range(0, ids.shape[0], per_call * G):
        out = torch_tower(sd, cfg, ids[i:i + per_call * G], None, dtype).float()
        out = F.normalize(out, dim=-1).reshape(-1, G, out.shape[-1]).mean(dim=1)
        rows.append(F.normalize(out, dim=-1))
    return torch.cat(rows)


def native_table(m, ids, G, per_call):
    return torch.cat([m.encode_groups(ids[i:i + per_call * G], G) for i in range(0, ids.shape[0], per_call * G)])


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    cfg = sa.SiglipTextConfig()
    lines = [f"text tower, SigLIP-base text shapes: vocab {cfg.vocab_size}, D {cfg.hidden_size}, {cfg.num_hidden_layers} layers, "
             f"{cfg.num_attention_heads} heads, I {cfg.intermediate_size}, L {cfg.max_position_embeddings}; {torch.cuda.get_device_name(0)}",
             "milliseconds per call: median (min) of the timed repetitions, HIP events; torch = the same operator sequence, same GPU, same process"]
    g = torch.Generator().manual_seed(0)
    ids8 = torch.randint(0, cfg.vocab_size, (8, 64), generator=g).to(dev)
    mask8 = (torch.arange(64)[None] < torch.tensor([64, 9, 12, 30, 5, 17, 22, 8])[:, None]).long().to(dev)
    labels, G = 400, 28
    per_call = max(1, PROMPTS_PER_CALL // G)
    ids_tab = torch.randint(0, cfg.vocab_size, (labels * G, 64), generator=g).to(dev)
    for mode, tdtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.manual_seed(1)
        m = sa.SiglipTextModel(cfg, compute_dtype=mode)
        for p in m.parameters():
            if p.dim() > 1:
                torch.nn.init.normal_(p, std=0.02)
        m.to(dev)
        sd = {k: v.detach() for k, v in m.state_dict().items()}
        with torch.no_grad():
            got = m(ids8, attention_mask=mask8)[1]
            want = torch_tower(sd, cfg, ids8, mask8, torch.float32)
            lines.append(f"[{mode}] 8 captions, pooled max-abs against torch fp32: {float((got - want).abs().max()):.3e} (max |ref| {float(want.abs().max()):.2f})")
            n_ms = timed(lambda: m(ids8, attention_mask=mask8), warmup=5, iters=30)
            t_ms = timed(lambda: torch_tower(sd, cfg, ids8, mask8, tdtype), warmup=5, iters=30)
            lines.append(f"[{mode}] per-step case, 8 captions x 64 tokens, masked: native {n_ms[0]:.3f} ({n_ms[1]:.3f}) ms   torch {tdtype} {t_ms[0]:.3f} ({t_ms[1]:.3f}) ms")
            n_ms = timed(lambda: native_table(m, ids_tab, G, per_call), warmup=1, iters=3)
            t_ms = timed(lambda: torch_table(sd, cfg, ids_tab, G, tdtype, per_call), warmup=1, iters=3)
            lines.append(f"[{mode}] class-table case, {labels} labels x {G} templates, {per_call * G} prompts per call: native {n_ms[0]:.1f} ({n_ms[1]:.1f}) ms   "
                         f"torch {tdtype} {t_ms[0]:.1f} ({t_ms[1]:.1f}) ms")
        del m
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "text_tower.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
