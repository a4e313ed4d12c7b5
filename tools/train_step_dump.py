"""One training step on seeded inputs, written to a file: the bit-identity check of a host-side change to the training step.

    python tools/train_step_dump.py --case base_lora --out a.pt [--root OTHER_TREE] [--staged]
    python tools/train_step_dump.py --compare a.pt b.pt

A case runs zero_grad, forward, the localization loss gradient, backward and one AdamW step in a fresh process and saves
last_hidden_state, pooler_output, the flat gradient buffer (as the backward left it), the parameters after the step and
sf_trainer_workspace_bytes (for the case's geometry and a sweep of others).  --root imports the package from another tree (a build of
the parent commit); --staged issues the backward one stage per call.  --compare names every tensor of two files that differs
(torch.equal) and exits non-zero if one does.  The training switches (SF_WGRAD_UNGROUPED, ...) are taken from the environment as usual."""
import argparse
import ctypes as C
import os
import sys

import torch

HD72W = dict(image_size=42, patch_size=14, num_frames=8, hidden_size=576, num_hidden_layers=2, num_attention_heads=8, intermediate_size=1072)
SO400M_LAYER = dict(image_size=196, patch_size=14, num_frames=4, hidden_size=1152, num_hidden_layers=1, num_attention_heads=16,
                    intermediate_size=4304)
# name -> (config overrides or None for SigLIP-base, lora, freeze_spatial, drop rates, B, T)
CASES = {
    "base_lora": (None, True, True, False, 8, 16),              # the benchmark's recipe: fused temporal, grouped, side stream
    "base_nolora": (None, False, False, False, 8, 16),
    "base_lora_unfrozen": (None, True, False, False, 8, 16),
    "base_drops": (None, True, True, True, 8, 16),              # hidden + attention dropout + drop_path: unfused, immediate launches
    "hd72w": (HD72W, True, True, False, 2, 8),                  # generic kernels, padded widths, shapes that do not group
    "so400m_layer": (SO400M_LAYER, True, True, False, 2, 4),    # one so400m-width layer: the workspace of widths that do not group
}
SWEEP = [(1, 1), (1, 16), (2, 8), (8, 16), (16, 16), (32, 4)]


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    bad = [k for k in a if (not torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] != b[k])]
    for k in a:
        print(f"  {k:20s} {'DIFFERS' if k in bad else 'equal'}")
    return 1 if bad or set(a) != set(b) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--staged", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.root))
    import streamformer_amd as sa
    import streamformer_amd._native as nat
    from streamformer_amd.configuration import StreamformerConfig
    from streamformer_amd.training import StreamformerTrainer

    kw, lora, freeze, drops, B, T = CASES[args.case]
    extra = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, drop_path_rate=0.1) if drops else {}
    cfg = (sa.siglip_base(add_lora_spatial=lora, **extra) if kw is None
           else StreamformerConfig(enable_causal_temporal=True, add_lora_spatial=lora, **kw, **extra))
    sd = sa.make_state_dict(cfg, seed=0, lora=lora)
    tr = StreamformerTrainer(cfg, sd, ["retrieval", "localization"], freeze_spatial=freeze, device="cuda:0", drop_path_seed=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    lab = torch.randn(20, cfg.hidden_size, generator=g)
    lab = (lab / lab.norm(dim=-1, keepdim=True)).cuda()
    ti = {"kind": "localization", "label_emb": lab, "labels": torch.randint(-1, 20, (B, T), generator=g).cuda()}
    tr.zero_grad()
    lhs, pooler = tr.forward(x)
    _, gp, _ = tr.loss_and_grad("localization", pooler, ti)
    if args.staged:
        for st in range(len(tr.stage_ranges)):
            nat.check(nat.lib.sf_trainer_backward(tr._h, gp.data_ptr(), None, tr.grads.data_ptr(), st, st, tr._ws.data_ptr(), tr._ws.numel(),
                                                  nat.current_stream_handle(tr.device)))
    else:
        tr.backward(gp)
    torch.cuda.synchronize()
    out = {"last_hidden_state": lhs.cpu(), "pooler_output": pooler.cpu(), "grads": tr.grads.cpu()}
    tr.optimizer_step(lr=1e-3)
    torch.cuda.synchronize()
    out["params_after_step"] = tr.params.cpu()
    n = C.c_size_t()
    ws = []
    for b, t in [(B, T)] + [bt for bt in SWEEP if bt[1] <= cfg.num_frames]:
        nat.check(nat.lib.sf_trainer_workspace_bytes(tr._h, b, t, C.byref(n)))
        ws.append((b, t, int(n.value)))
    out["workspace_bytes"] = ws
    torch.save(out, args.out)
    print(f"{args.case}: wrote {args.out}; workspace_bytes {ws[0][2]}; |grads| {float(out['grads'].norm()):.6e}", flush=True)


if __name__ == "__main__":
    main()
