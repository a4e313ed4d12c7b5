"""CPU: multi-scale deformable attention without a GPU — the fp64 restatement (tests/msda_oracle.py) against fixture F21 (the reference's
own MSDeformAttn and ms_deform_attn_core_pytorch in fp64), the module's parameter tree and initialisation, the refusals of the C entry
points (nothing is launched), the CPU-tensor error and the stand-in for the reference's compiled extension."""
import ctypes as C
import functools

import pytest
import torch

from tests import msda_oracle as MO
from tests.helpers import maxabs

EPS64 = 2.0 ** -52
ROUNDING = 1e4 * EPS64      # "fp64 rounding": two fp64 evaluations in different summation orders, results of magnitude ~1


@functools.lru_cache(maxsize=None)
def _gold():
    return MO.load_golden()


def _t(name):
    return torch.from_numpy(_gold()[name])


def _close(got, want):
    return maxabs(got, want) <= ROUNDING * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("name", list(MO.CORE_CASES))
def test_oracle_core_matches_f21(name):
    c = MO.CORE_CASES[name]
    value, loc, w, go = (_t(f"{name}.{k}") for k in ("value", "loc", "w", "grad_out"))
    assert MO.away_from_integers(loc, c["shapes"])
    for fn in (MO.core, MO.core_grid_sample):
        out, gv, gl, gw = MO.core_with_grads(fn, value.double(), c["shapes"], loc.double(), w.double(), go.double())
        for got, key in ((out, "out"), (gv, "grad_value"), (gl, "grad_loc"), (gw, "grad_w")):
            assert _close(got, _t(f"{name}.{key}")), (fn.__name__, key, maxabs(got, _t(f"{name}.{key}")))
    # the drawn inputs are the stored ones
    for got, key in zip(MO.make_core_inputs(c), ("value", "loc", "w", "grad_out")):
        assert torch.equal(got, _t(f"{name}.{key}")), key


def _module_inputs(name):
    g = _gold()
    query, flat, ref, go = (_t(f"{name}.{k}").float() for k in ("query", "input_flatten", "reference_points", "grad_out"))
    mask = _t(f"{name}.mask") if f"{name}.mask" in g else None
    return query, flat, ref, mask, go


@pytest.mark.parametrize("name", list(MO.MODULE_CASES))
def test_oracle_module_matches_f21(name):
    c = MO.MODULE_CASES[name]
    assert int(_gold()[f"{name}.seed"]) == c["seed"]
    sd = MO.make_weights(c)
    query, flat, ref, mask, go = _module_inputs(name)
    assert (mask is not None) == c["mask"]
    if mask is not None:      # one level wholly masked
        assert bool(mask[1, MO.level_starts(c["shapes"])[-1]:].all())
    if c["grads"]:
        loc = MO.module(sd, c, query, flat, ref, mask, parts=True)[4]
        assert MO.away_from_integers(loc, c["shapes"])
        out, grads = MO.module_with_grads(sd, c, query, flat, ref, mask, go)
        for k, g in grads.items():
            assert _close(g, _t(f"{name}.grad.{k}")), (k, maxabs(g, _t(f"{name}.grad.{k}")))
    else:
        out = MO.module(sd, c, query, flat, ref, mask)
    assert _close(out, _t(f"{name}.out")), maxabs(out, _t(f"{name}.out"))


@pytest.mark.parametrize("name", list(MO.MODULE_CASES))
def test_module_parameter_tree_and_init(name):
    import streamformer_amd as sa
    c = MO.MODULE_CASES[name]
    keys = [str(k) for k in _gold()[f"{name}.keys"]]
    m = sa.MSDeformAttn(c["d_model"], len(c["shapes"]), c["heads"], c["P"])
    assert list(m.state_dict().keys()) == keys
    assert [k for k, _ in m.named_parameters()] == keys
    assert torch.equal(m.sampling_offsets.bias.detach(), _t(f"{name}.init_offsets_bias")), "the ring-shaped bias grid differs"
    assert not m.sampling_offsets.weight.any() and not m.attention_weights.weight.any() and not m.attention_weights.bias.any()
    assert not m.value_proj.bias.any() and not m.output_proj.bias.any()
    bound = (6.0 / (2 * c["d_model"])) ** 0.5      # xavier_uniform_
    for w in (m.value_proj.weight, m.output_proj.weight):
        assert float(w.detach().abs().max()) <= bound and float(w.detach().std()) > 0.4 * bound
    sd = MO.make_weights(c)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]) and v.shape == sd[k].shape


def test_ratio_is_ignored():
    import streamformer_amd as sa
    a, b = sa.MSDeformAttn(64, 2, 2, 2, ratio=0.5), sa.MSDeformAttn(64, 2, 2, 2)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}
    assert a.value_proj.out_features == 64 and a.output_proj.in_features == 64
    with pytest.raises(ValueError):
        sa.MSDeformAttn(64, 2, 3, 2)
    with pytest.raises(ValueError):
        sa.MSDeformAttn(64, 2, 2, 2, compute_dtype="fp8")


def _call(nat, which, D=8, L=2, shapes=(2, 3, 1, 2), starts=(0, 6), S=8, null=None, P=2, M=2, Lq=3, N=2, ref_dim=2):
    """One refused call: fake non-null device addresses (nothing may be dereferenced or launched), `null` names the pointer to zero."""
    hw, st = (C.c_int32 * len(shapes))(*shapes), (C.c_int32 * len(starts))(*starts)
    ptr = {k: 0x1000 * (i + 1) for i, k in enumerate(("value", "loc", "w", "out", "go", "gv", "gl", "gw", "ref"))}
    if null in ptr:
        ptr[null] = 0
    hw_p, st_p = (None if null == "shapes" else hw), (None if null == "starts" else st)
    if which == "forward":
        return nat.lib.sf_op_msda_forward(ptr["value"], hw_p, st_p, ptr["loc"], ptr["w"], ptr["out"], N, S, M, D, Lq, L, P, None)
    if which == "fused":
        return nat.lib.sf_op_msda_forward_fused(ptr["value"], None, hw_p, st_p, ptr["loc"], M * L * P * 3, ptr["w"], M * L * P * 3, ptr["ref"], ref_dim,
                                                ptr["out"], N, S, M, D, Lq, L, P, None)
    return nat.lib.sf_op_msda_backward(ptr["value"], hw_p, st_p, ptr["loc"], ptr["w"], ptr["go"], ptr["gv"], ptr["gl"], ptr["gw"], N, S, M, D, Lq, L, P, None)


@pytest.mark.parametrize("which", ["forward", "fused", "backward"])
def test_entry_points_refuse_before_launch(which):
    import streamformer_amd._native as nat

    def refused(field, **kw):
        assert _call(nat, which, **kw) == nat.SF_ERR_INVALID, (field, kw)
        msg = nat.lib.sf_last_error().decode()
        assert field in msg and f"sf_op_msda_{'forward_fused' if which == 'fused' else which}" in msg, msg

    refused("D = 12", D=12)
    refused("D = 136", D=136)
    refused("D = 0", D=0)
    refused("L = 9", L=9, shapes=(1, 1) * 9, starts=tuple(range(9)), S=9)
    refused("L = 0", L=0)
    refused("P = 9", P=9)
    refused("sum to 8 pixels, S = 9", S=9)
    refused("sum to 8 pixels, S = 7", S=7, starts=(0, 5))
    refused("level_start_index[1]", starts=(0, 7))
    refused("spatial_shapes[0]", shapes=(0, 3, 1, 2))
    refused("Lq = 0", Lq=0)
    refused("null", null="shapes")
    refused("null", null="starts")
    nulls = {"forward": ("value", "loc", "w", "out"), "fused": ("value", "loc", "w", "ref", "out"), "backward": ("value", "loc", "w", "go", "gv", "gl", "gw")}
    for name in nulls[which]:
        refused("null", null=name)
    if which == "fused":
        refused("ref_dim = 3", ref_dim=3)


def test_cpu_tensors_raise():
    import streamformer_amd as sa
    c = MO.MODULE_CASES["tiny"]
    m = sa.MSDeformAttn(c["d_model"], len(c["shapes"]), c["heads"], c["P"])
    query, flat, ref, mask, _ = MO.make_module_inputs(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(query, ref, flat, torch.tensor(c["shapes"]), torch.tensor(MO.level_starts(c["shapes"])), mask)
    cc = MO.CORE_CASES["c0"]
    value, loc, w, _ = MO.make_core_inputs(cc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sa.ms_deform_attn(value, cc["shapes"], None, loc, w)


def test_compiled_op_stand_in():
    import streamformer_amd as sa
    op = sa.as_compiled_op()
    assert op.__name__ == "MultiScaleDeformableAttention"
    assert callable(op.ms_deform_attn_forward) and callable(op.ms_deform_attn_backward)
    assert sa.msda.as_compiled_op is sa.as_compiled_op and issubclass(sa.MSDeformAttnFunction, torch.autograd.Function)
