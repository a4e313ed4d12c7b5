"""Time per step of the native online-action detector against the reference's operator sequence in torch, on the same GPU, in the same process.

    python tools/oad_bench.py            # writes profiles/oad.txt

Shapes of the THUMOS recipe: d_in 768, d_model 1024, 4 heads of 256, FFN 1024, L 64 long samples, W 32 work frames, ENC_MODULE
[[16, 1, True], [32, 2, True]], DEC_MODULE [-1, 2, True], 22 classes, random weights; 1 and 8 streams; both compute modes.  Two steady-state
steps are timed: one that pushes a long sample (stage 0 runs) and one that does not (the cached compressed memory is reused).

The torch side is what LSTRStream.stream_inference does per step once its caches are warm: the feature heads, the new sample's k / v
projection and the ``torch.cat`` roll of the k, v and q.k caches, softmax(q.k + q.k_pos + mask)(v + v_pos), then the later stages and the
work decoder on the whole work window, in fp32 next to the accurate mode and with bf16 weights / activations (no autocast) next to the bf16
mode.  The reference handles one stream per model (its caches and ``view(-1, bsz * heads, head_dim)`` break at bsz > 1), so n streams are n
such steps in a row.

Method: every timed window is a batch of steps between two HIP events (at least ~50 ms of work), native and torch windows alternate, the
median (min) over the windows is reported, everything is warmed up first; the scores of both sides are compared before anything is timed.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import streamformer_amd as sa  # noqa: E402
from tools._timing import compare  # noqa: E402

CFG = sa.OADConfig()      # the THUMOS shapes are the defaults
D, H, L, W_, DIN = CFG.d_model, CFG.NUM_HEADS, CFG.LONG_MEMORY_NUM_SAMPLES, CFG.WORK_MEMORY_NUM_SAMPLES, CFG.VISUAL_SIZE


def heads(t):
    return t.reshape(t.shape[0], H, D // H).transpose(0, 1)


def attend(q, k, v, mask=None):
    s = torch.bmm(heads(q) * (D // H) ** -0.5, heads(k).transpose(1, 2))
    if mask is not None:
        s = s + mask
    return torch.bmm(F.softmax(s, dim=-1), heads(v)).transpose(0, 1).reshape(q.shape[0], D)


class TorchStream:
    """One stream of the reference's stream path with warm caches (weights W on the device in the run's dtype)."""

    def __init__(self, W, pe):
        self.W, self.pe = W, pe
        p = "enc_modules.0.layers.0."
        w, b = W[p + "multihead_attn.in_proj_weight"], W[p + "multihead_attn.in_proj_bias"]
        self.tgt0 = self.self_attn(p, W["enc_queries.0.weight"], None)
        self.q0 = F.linear(self.tgt0, w[:D], b[:D])
        self.k_pos, self.v_pos = F.linear(pe[:L], w[D:2 * D], b[D:2 * D]), F.linear(pe[:L], w[2 * D:], b[2 * D:])
        self.kpos_w = torch.bmm(heads(self.q0) * (D // H) ** -0.5, heads(self.k_pos).transpose(1, 2))
        self.causal = torch.triu(torch.full((W_, W_), float("-inf"), device=pe.device, dtype=pe.dtype), diagonal=1)
        self.k = self.v = self.k_w = self.mem0 = None

    def ln(self, x, p):
        return F.layer_norm(x, (D,), self.W[p + ".weight"], self.W[p + ".bias"])

    def head(self, which, x):
        p = f"feature_head_{which}.visual_linear."
        return F.relu(self.ln(F.linear(x, self.W[p + "0.weight"], self.W[p + "0.bias"]), p + "1"))

    def self_attn(self, p, x, mask):
        qkv = F.linear(x, self.W[p + "self_attn.in_proj_weight"], self.W[p + "self_attn.in_proj_bias"])
        y = F.linear(attend(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], mask), self.W[p + "self_attn.out_proj.weight"], self.W[p + "self_attn.out_proj.bias"])
        return self.ln(x + y, p + "norm1")

    def cross_attn(self, p, x, mem):
        w, b = self.W[p + "multihead_attn.in_proj_weight"], self.W[p + "multihead_attn.in_proj_bias"]
        ctx = attend(F.linear(x, w[:D], b[:D]), F.linear(mem, w[D:2 * D], b[D:2 * D]), F.linear(mem, w[2 * D:], b[2 * D:]))
        return self.ln(x + F.linear(ctx, self.W[p + "multihead_attn.out_proj.weight"], self.W[p + "multihead_attn.out_proj.bias"]), p + "norm2")

    def ffn(self, p, x, norm):
        y = F.linear(F.relu(F.linear(x, self.W[p + "linear1.weight"], self.W[p + "linear1.bias"])), self.W[p + "linear2.weight"], self.W[p + "linear2.bias"])
        return self.ln(x + y, p + norm)

    def step(self, work, long=None, mask=None):
        p = "enc_modules.0.layers.0."
        if long is not None:
            w = self.W[p + "multihead_attn.in_proj_weight"]
            x = self.head("long", long)
            k_new, v_new = F.linear(x, w[D:2 * D]), F.linear(x, w[2 * D:])
            qs = heads(self.q0) * (D // H) ** -0.5
            if self.k is None:
                self.k, self.v = k_new, v_new
                self.k_w = torch.bmm(qs, heads(self.k).transpose(1, 2))
            else:
                self.k, self.v = torch.cat((self.k[1:], k_new)), torch.cat((self.v[1:], v_new))
                self.k_w = torch.cat((self.k_w[:, :, 1:], torch.bmm(qs, heads(k_new).transpose(1, 2))), dim=-1)
            s = self.k_w + self.kpos_w
            if mask is not None:
                s = s + mask
            ctx = torch.bmm(F.softmax(s, dim=-1), heads(self.v + self.v_pos)).transpose(0, 1).reshape(-1, D)
            x = self.ln(self.tgt0 + F.linear(ctx, self.W[p + "multihead_attn.out_proj.weight"], self.W[p + "multihead_attn.out_proj.bias"]), p + "norm2")
            self.mem0 = self.ln(self.ffn(p, x, "norm3"), "enc_modules.0.norm")
        mem = self.mem0
        x = self.W["enc_queries.1.weight"]
        for i in range(2):
            q = f"enc_modules.1.layers.{i}."
            x = self.ffn(q, self.cross_attn(q, self.self_attn(q, x, None), mem), "norm3")
        mem = self.ln(x, "enc_modules.1.norm")
        x = self.head("work", work) + self.pe[L:L + W_]
        for i in range(2):
            q = f"dec_modules.layers.{i}."
            x = self.ffn(q, self.cross_attn(q, self.self_attn(q, x, self.causal), mem), "norm3")
        return F.linear(self.ln(x, "dec_modules.norm"), self.W["classifier.weight"], self.W["classifier.bias"])


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lines = [f"online action detection, one step: d_in {DIN}, d_model {D}, {H} heads of {D // H}, FFN {CFG.DIM_FEEDFORWARD}, L {L}, W {W_}, "
             f"ENC_MODULE {CFG.ENC_MODULE}, DEC_MODULE {CFG.DEC_MODULE}, {CFG.NUM_CLASSES} classes; {torch.cuda.get_device_name(0)}",
             "milliseconds per step: median (min) over alternating windows of >= 50 ms between HIP events; torch = the reference's stream path "
             "with warm caches, one stream at a time, same GPU, same process"]
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        seed = sa.OnlineActionDetector(CFG)
        sd = {}
        for k, v in seed.state_dict().items():
            if k == "pos_encoding.pe":
                continue
            if v.dim() == 2:
                sd[k] = torch.randn(v.shape, generator=g) / (1.0 if k.startswith("enc_queries") else v.shape[1] ** 0.5)
            else:
                sd[k] = (1.0 if ("norm" in k or ".visual_linear.1." in k) and k.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g)
        pe = seed.pos_encoding.pe[:L + W_, 0]
        mask = torch.zeros(L)
        mask[:5] = float("-inf")
        for mode, tdtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            det = sa.OnlineActionDetector(CFG, compute_dtype=mode)
            det.load_state_dict(sd, strict=False)
            det.to(dev)
            Wt = {k: v.to(dev, tdtype) for k, v in sd.items()}
            for n in (1, 8):
                work = torch.randn(n, W_, DIN, generator=g).to(dev)
                window, new = torch.randn(n, L, DIN, generator=g).to(dev), torch.randn(n, 1, DIN, generator=g).to(dev)
                state = det.new_state(n)
                refs = [TorchStream(Wt, pe.to(dev, tdtype)) for _ in range(n)]
                mk, mk_t = mask.to(dev)[None].expand(n, L).contiguous(), mask.to(dev, tdtype)
                got = det.step(work, window, mk, state=state)
                want = torch.stack([r.step(work[i].to(tdtype), window[i].to(tdtype), mk_t) for i, r in enumerate(refs)]).float()
                got2 = det.step(work, new, mk, state=state)
                want2 = torch.stack([r.step(work[i].to(tdtype), new[i].to(tdtype), mk_t) for i, r in enumerate(refs)]).float()
                lines.append(f"[{mode}] {n} stream(s): scores max-abs against torch {tdtype}: first step {float((got - want).abs().max()):.3e}, "
                             f"pushed sample {float((got2 - want2).abs().max()):.3e} (max |ref| {float(want2.abs().max()):.2f})")
                wt, nt = work.to(tdtype), new.to(tdtype)
                for label, lg in (("long sample pushed", new), ("no long sample", None)):
                    def native():
                        return det.step(work, lg, mk if lg is not None else None, state=state)

                    def reference():
                        return [r.step(wt[i], None if lg is None else nt[i], mk_t if lg is not None else None) for i, r in enumerate(refs)]

                    nat_ms, t_ms = compare(native, reference, warmup=5, windows=9, target_ms=50.0)
                    lines.append(f"[{mode}] {n} stream(s), {label}: native {nat_ms[0]:.3f} ({nat_ms[1]:.3f}) ms   torch {tdtype} {t_ms[0]:.3f} ({t_ms[1]:.3f}) ms   "
                                 f"torch / native {t_ms[0] / nat_ms[0]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "oad.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
