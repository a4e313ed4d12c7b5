"""Oracle of the CTVIS contrastive loss (streamformer_amd/cl_plugin.py): ``CTCLPlugin.get_reid_loss``, ``TrainTracklet`` and ``loss_reid``
of the reference's ``ctvis/modeling/cl_plugin/ct_cl_plugin.py`` restated in torch, in the reference's operator order and in any dtype, on
any device, plus the planted scenario of fixture F28 (tools/make_golden_cl_plugin.py pins this file to the reference).

What is kept, quirks included (line numbers of ct_cl_plugin.py):
  layout     pred_embeds [B F, Q, C], image n = b F + f (:226-242); one matcher call per frame position over the B images of it (:248-255);
             gt2query[b][f][i] = src[argsort(tgt)][i] (:278-279); a video's instance count is frame 0's (:283); valid = gt_ids != -1.
  bank fill  valid: anchor = the matched row, negatives = sorted(random.sample(set(range(nn + 1)) - {query}, nn)) rows of that frame: the
             population is the FIRST nn + 1 queries, not Q (:295-296).  Invalid: anchor None, negatives all Q rows.
  sg         first present frame copies; later present frames sim = sum_j cos(e_j, p) / exist_frames, beta = max(0, sim) (the builtin: the
             tensor sim when sim > 0, so the gradient flows through beta, else the constant 0), sg = (1 - beta) sg + beta p; absent
             frames repeat the previous sg (:43-85).
  items      frame f >= 1, instance valid at f.  exist_before(f): positive = sg_list[f - 1] when momentum_embed and one
             np.random.rand() > 0.5 (drawn only then), else the last present embedding before f.  Otherwise exist_after(f) AS WRITTEN,
             ``f != (number of None entries after f)`` (quirk 1: not "some later frame has it"): the first present embedding after f, and
             no item when the search finds none.  Negatives: the bank's of frame f - 1 (quirk 2: the sampled rows if the instance was
             valid THERE, all Q rows if not) (:87-112, :306-336).
  loss       d = [p; N] a; contras = logsumexp([d_neg - d_pos, 0]); aux = mean((cos([p; N], a) - label)^2); both summed over the items and
             divided by their number; without items both are pred_embeds.sum() * 0 (:426-470).

Every input is a pure function of a seed (numpy PCG64 and arithmetic, exactly representable in fp32).  Matched rows follow a direction per
instance, so every sim is far from 0; ``flip`` turns one frame's embedding round (one negative sim, beta = 0).  ``SIM_MARGIN`` is the
condition on every other |sim| that the generator and tests/test_cl_plugin_cpu.py check.
"""
import random

import numpy as np
import torch
import torch.nn.functional as F

from tests import criterion_oracle as CO

SIM_MARGIN = 1e-2
WEIGHTS = {"loss_reid": 2.0, "loss_aux_reid": 3.0}
BRANCHES = ("fill_valid", "fill_invalid", "anchor_inside", "anchor_outside", "sample_noop", "first_copy", "beta_zero", "beta_positive",
            "absent_repeat", "pos_sg", "pos_last_coin", "pos_last_no_momentum", "pos_after", "after_quirk_false", "after_search_none",
            "neg_sampled", "neg_all", "never_present", "video_without_instances", "no_item_single_frame")

# valid[b][i] is the instance's present / absent sequence over the frames
CASES = {
    # Q > nn + 1: matched queries inside and outside the first nn + 1
    "main": dict(seed=4101, B=2, F=5, Q=12, C=256, nn=9, momentum=True, draw_seed=11, flip=((0, 0, 2),),
                 valid=(("11111", "01111", "01011", "01000", "10110", "00000", "01001"), ("11111", "00001", "11011"))),
    # Q = nn + 1 (sampling is a no-op), C = 40, a video without instances
    "tight": dict(seed=4102, B=2, F=5, Q=8, C=40, nn=7, momentum=True, draw_seed=5, flip=(),
                  valid=(("11111", "10110", "00100"), ())),
    "nomom": dict(seed=4103, B=2, F=2, Q=8, C=40, nn=7, momentum=False, draw_seed=3, flip=(), valid=(("11", "01"), ("11",))),
    "single": dict(seed=4104, B=2, F=1, Q=8, C=40, nn=7, momentum=True, draw_seed=3, flip=(), valid=(("1", "0"), ("1",))),
}
# train_loss end to end: logits and masks of tests/criterion_oracle.py's scenario (one image per (video, frame)), embeddings planted on
# the assignment they give
E2E = dict(seed=4105, B=2, F=2, Q=12, C=256, nn=9, momentum=True, draw_seed=7, flip=(), valid=(("11", "01", "10"), ("11", "11")),
           crit=dict(CO.BASE, seed=4106, L=1, Q=12, K=64))


_MATCHED = {}           # the end-to-end scenario's fp64 assignment, computed once


def instances(case, b):
    return len(case["valid"][b])


def valid_flags(case):
    """valid[b][f][i] as nested lists of bool."""
    return [[[case["valid"][b][i][f] == "1" for i in range(instances(case, b))] for f in range(case["F"])] for b in range(case["B"])]


def crit_case(case):
    """The criterion_oracle case of the end-to-end scenario: image n = b F + f has the G_b targets of its video."""
    g = tuple(instances(case, b) for b in range(case["B"]) for _ in range(case["F"]))
    return dict(case["crit"], B=case["B"] * case["F"], G=g, tgt=((96, 160),) * len(g))


def match_draws(case):
    """The matcher's planted point draws of the end-to-end scenario in the reference's order: position f outer, image b inner."""
    rng = np.random.default_rng(case["seed"] + 100000)
    K = case["crit"]["K"]
    return [np.minimum(rng.random((1, K, 2), dtype=np.float32), np.float32(1.0 - 2.0 ** -24)) for _ in range(case["F"] * case["B"])]


def matcher_indices(case, dtype=torch.float64, device="cpu"):
    """The reference's per-position matcher calls on the end-to-end scenario: (indices_list[f][b] = (src, tgt), cost matrices in that order)."""
    cc = crit_case(case)
    outputs, targets, _ = CO.tensors(cc, dtype, device)
    queue = CO.Queue(match_draws(case), dtype)
    Fn, B = case["F"], case["B"]
    indices, costs = [], []
    for f in range(Fn):
        sel = [b * Fn + f for b in range(B)]
        layer = {"pred_logits": outputs["pred_logits"][sel], "pred_masks": outputs["pred_masks"][sel]}
        with torch.no_grad():
            c = CO.cost_matrices(cc, layer, [targets[n] for n in sel], queue)
        costs.append(c)
        indices.append(CO.assign(c))
    return indices, costs


def scripted_indices(case):
    """indices_list[f][b] = (src sorted, tgt) as scipy's solver would give them: a seeded injection of the G_b instances into the queries."""
    if "crit" in case:
        if case["seed"] not in _MATCHED:
            _MATCHED[case["seed"]] = matcher_indices(case)[0]
        return _MATCHED[case["seed"]]
    rng = np.random.default_rng(case["seed"] + 7)
    out = []
    for f in range(case["F"]):
        per = []
        for b in range(case["B"]):
            g = instances(case, b)
            src = rng.permutation(case["Q"])[:g]
            order = np.argsort(src)
            per.append((torch.as_tensor(src[order], dtype=torch.int64), torch.as_tensor(np.arange(g)[order], dtype=torch.int64)))
        out.append(per)
    return out


def gt2query_of(indices_list, B):
    """gt2query[b][f] = src[argsort(tgt)] as a list of ints."""
    return [[[int(q) for q in per[b][0][torch.sort(per[b][1])[1]]] for per in indices_list] for b in range(B)]


def embeddings(case):
    """pred_embeds [B F, Q, C] fp32 numpy: noise everywhere; the matched row of instance i at frame f follows the instance's direction
    (turned round where ``flip`` says so), scaled so that the dot products of an item spread over a few units."""
    rng = np.random.default_rng(case["seed"])
    B, Fn, Q, C = case["B"], case["F"], case["Q"], case["C"]
    scale = np.float32(3.2 / np.sqrt(C))
    e = rng.standard_normal((B * Fn, Q, C)).astype(np.float32) * scale
    g2q = gt2query_of(scripted_indices(case), B)
    for b in range(B):
        for i in range(instances(case, b)):
            base = rng.standard_normal(C).astype(np.float32)
            for f in range(Fn):
                sign = np.float32(-1.0 if (b, i, f) in case["flip"] else 1.0)
                strength = np.float32(rng.uniform(0.8, 1.3))
                e[b * Fn + f, g2q[b][f][i]] = (sign * strength * base + np.float32(0.5) * rng.standard_normal(C).astype(np.float32)) * scale
    return e


def checksum(case):
    return np.asarray([float(np.abs(embeddings(case)).sum(dtype=np.float64)), float(sum(sum(int(q) for q in f) for b in gt2query_of(scripted_indices(case), case["B"]) for f in b))])


def seeded_hooks(seed):
    """The reference's own draws: ``random.sample`` and ``np.random.rand`` after seeding both with ``seed``."""
    random.seed(seed)
    np.random.seed(seed)
    return (lambda population, k: random.sample(population, k)), (lambda: np.random.rand())


# ---------------------------------------------------------------------------------------------------
# the reference's operators
# ---------------------------------------------------------------------------------------------------
def exist_before(present, f):
    return f != sum(1 for p in present[:f] if not p)


def exist_after(present, f):
    return f != sum(1 for p in present[f + 1:] if not p)                   # the reference's expression as written


def reid_loss(embeds, Fn, nn, gt2query, valid, momentum=True, sample=None, coin=None):
    """get_reid_loss + loss_reid on pred_embeds [B F, Q, C].  Returns a dict: plan (one tuple per item: video, instance, frame, anchor
    query, positive kind (0 an embedding, 1 sg), positive frame, negative queries of frame - 1), items [(dot_product, cosine_similarity,
    label)], sg[(b, i)] (per frame a tensor or None), sim[(b, i, f)], losses (loss_reid, loss_aux_reid), counts of the branches taken."""
    sample = sample or (lambda population, k: random.sample(population, k))
    coin = coin or (lambda: np.random.rand())
    counts = dict.fromkeys(BRANCHES, 0)
    B, Q = embeds.shape[0] // Fn, embeds.shape[1]
    plan, items, sg_all, sim_all = [], [], {}, {}
    for b in range(B):
        G = len(valid[b][0])
        counts["video_without_instances"] += G == 0
        frames = [embeds[b * Fn + f] for f in range(Fn)]
        reid = [[None] * Fn for _ in range(G)]              # the bank: per instance per frame the anchor [1, C] or None
        negs = [[None] * Fn for _ in range(G)]              # and the negative queries
        sg_list = [[None] * Fn for _ in range(G)]
        for f in range(Fn):
            for i in range(G):
                if valid[b][f][i]:
                    q = gt2query[b][f][i]
                    counts["fill_valid"] += 1
                    counts["anchor_inside" if q <= nn else "anchor_outside"] += 1
                    counts["sample_noop"] += Q == nn + 1
                    reid[i][f] = frames[f][q][None, ...]
                    negs[i][f] = sorted(sample(tuple(set(range(nn + 1)) - set([q])), nn))
                else:
                    counts["fill_invalid"] += 1
                    negs[i][f] = list(range(Q))
                # TrainTracklet.update
                p = reid[i][f]
                before = [e for e in reid[i][:f] if e is not None]
                if p is None:
                    sg_list[i][f] = sg_list[i][f - 1] if f else None
                    counts["absent_repeat"] += f > 0 and sg_list[i][f] is not None
                elif not before:
                    sg_list[i][f] = p
                    counts["first_copy"] += 1
                else:
                    allp = torch.cat(before, dim=0)
                    sim = torch.sum(torch.einsum("bc,c->b", F.normalize(allp, dim=-1), F.normalize(p.squeeze(), dim=-1))) / len(before)
                    beta = max(0, sim)
                    counts["beta_positive" if sim > 0 else "beta_zero"] += 1
                    sim_all[(b, i, f)] = sim
                    sg_list[i][f] = (1 - beta) * sg_list[i][f - 1] + beta * p
        for f in range(1, Fn):
            for i in range(G):
                if reid[i][f] is None:
                    continue
                present = [e is not None for e in reid[i]]
                kind, pf, pos = 0, -1, None
                if exist_before(present, f):
                    if momentum and coin() > 0.5:
                        kind, pf, pos = 1, f - 1, sg_list[i][f - 1]
                        counts["pos_sg"] += 1
                    else:
                        pf = max(j for j in range(f) if present[j])
                        pos = reid[i][pf]
                        counts["pos_last_coin" if momentum else "pos_last_no_momentum"] += 1
                elif exist_after(present, f):
                    later = [j for j in range(f + 1, Fn) if present[j]]
                    if later:
                        pf, pos = later[0], reid[i][later[0]]
                        counts["pos_after"] += 1
                    else:
                        counts["after_search_none"] += 1
                else:
                    counts["after_quirk_false"] += 1
                if pos is None:
                    continue
                counts["neg_sampled" if present[f - 1] else "neg_all"] += 1
                anchor = reid[i][f]
                pos_neg = torch.cat([pos, frames[f - 1][negs[i][f - 1]]], dim=0)
                label = pos_neg.new_zeros((pos_neg.shape[0],), dtype=torch.int64)
                label[:1] = 1
                dot = torch.einsum("ac,kc->ak", [pos_neg, anchor])
                cos = torch.einsum("ac,kc->ak", [F.normalize(pos_neg, dim=1), F.normalize(anchor, dim=1)])
                plan.append((b, i, f, gt2query[b][f][i], kind, pf, tuple(negs[i][f - 1])))
                items.append((dot, cos, label))
        for i in range(G):
            sg_all[(b, i)] = sg_list[i]
            counts["never_present"] += all(e is None for e in reid[i])
    counts["no_item_single_frame"] += Fn == 1
    if not items:
        zero = embeds.sum() * 0
        return dict(plan=plan, items=items, sg=sg_all, sim=sim_all, losses=(zero, embeds.sum() * 0), counts=counts)
    contras, aux = 0, 0
    for dot, cos, label in items:
        pred = dot.permute(1, 0)
        x = F.pad(pred[:, 1:] - pred[:, :1], (0, 1), "constant", 0)
        contras = contras + torch.logsumexp(x, dim=1)
        aux = aux + (torch.abs(cos.permute(1, 0) - label.unsqueeze(0)) ** 2).mean()
    return dict(plan=plan, items=items, sg=sg_all, sim=sim_all, losses=(contras.sum() / len(items), aux / len(items)), counts=counts)


def run(case, dtype=torch.float64, device="cpu", grad=False, hooks=None):
    """The whole loss on a scenario with the reference's seeded draws (or ``hooks`` = (sample, coin)).  Adds to reid_loss's dict: embeds
    (the leaf), weighted (the dict train_loss returns), total (their sum), gt2query, valid."""
    e = torch.tensor(embeddings(case), dtype=dtype, device=device, requires_grad=grad)
    g2q, valid = gt2query_of(scripted_indices(case), case["B"]), valid_flags(case)
    sample, coin = hooks or seeded_hooks(case["draw_seed"])
    r = reid_loss(e, case["F"], case["nn"], g2q, valid, case["momentum"], sample, coin)
    r["weighted"] = {k: v * WEIGHTS[k] for k, v in zip(("loss_reid", "loss_aux_reid"), r["losses"])}
    r["total"] = r["weighted"]["loss_reid"] + r["weighted"]["loss_aux_reid"]
    r.update(embeds=e, gt2query=g2q, valid=valid)
    if grad:
        r["total"].backward()
    return r


def track_ids(case):
    """The (video, instance) pairs in the order of the native plan's tracks."""
    return [(b, i) for b in range(case["B"]) for i in range(instances(case, b))]


def plan_arrays(plan):
    """A plan as arrays: items int64 [I, 6] (video, instance, frame, anchor query, positive kind, positive frame), the negative queries
    concatenated, and their start per item [I + 1]."""
    items = np.asarray([p[:6] for p in plan], np.int64).reshape(-1, 6)
    start = np.cumsum([0] + [len(p[6]) for p in plan]).astype(np.int64)
    neg = np.asarray([q for p in plan for q in p[6]], np.int64)
    return items, neg, start


def sg_array(case, sg):
    """sg as [tracks, F, C] float64 with NaN rows where the reference holds None."""
    ids = track_ids(case)
    out = np.full((len(ids), case["F"], case["C"]), np.nan)
    for t, key in enumerate(ids):
        for f, v in enumerate(sg[key]):
            if v is not None:
                out[t, f] = v.detach().double().cpu().numpy().reshape(-1)
    return out


def min_abs_sim(sim, skip=()):
    vals = [abs(float(v)) for k, v in sim.items() if k not in skip]
    return min(vals) if vals else float("inf")
