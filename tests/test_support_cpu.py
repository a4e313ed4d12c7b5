"""The shared test vocabulary itself (tests/helpers.py, tests/oracle_ops.py), on the CPU: five oracles and a dozen test files lean on these
definitions, so a wrong one would weaken every bound at once."""
import pytest
import torch

from tests.helpers import EPS32, MARGIN, check_against_floor, cosine, fp32_floor, guarded, randn, read_guarded, rel_l2, rel_max
from tests.oracle_ops import bf16_round, operand_linear


# ------------------------------------------------------------------------------------------------
# the operand model
# ------------------------------------------------------------------------------------------------
def _operands():
    return randn(1, 7, 64).double(), randn(2, 5, 64).double(), randn(3, 5).double()


def test_operand_linear_exact_and_bf16_modes_are_the_plain_products():
    x, w, b = _operands()
    assert torch.equal(operand_linear(x, w, b, False), x @ w.t() + b)
    assert torch.equal(operand_linear(x, w, b), x @ w.t() + b)
    assert torch.equal(operand_linear(x, w, None, False), x @ w.t())
    assert torch.equal(operand_linear(x, w, b, True), bf16_round(x) @ bf16_round(w).t() + b)


def test_operand_linear_x3_is_within_its_derived_bound_and_closer_than_one_rounding():
    """One bf16 rounding loses at most 2^-9 relative, so x = xh + xl + rx with |xl| <= 2^-9 |x| and |rx| <= 2^-18 |x| (the same for w).
    x w - (xh wh + xh wl + xl wh) = xl wl + rx w + x rw - (second-order terms): three terms of at most 2^-18 |x| |w| each, the rest far
    below a fourth; summed over k that is 4 * 2^-18 = 2^-16 times |x| @ |w|^T elementwise."""
    x, w, b = _operands()
    exact = x @ w.t() + b
    err3 = (operand_linear(x, w, b, "x3") - exact).abs()
    err1 = (operand_linear(x, w, b, True) - exact).abs()
    assert bool((err3 <= 2.0 ** -16 * (x.abs() @ w.abs().t())).all()), float(err3.max())
    assert float(err3.max()) > 0.0          # the planes are not exact: fp64 operands do not fit two bf16 values
    assert float(err3.max()) < float(err1.max()) and float(err3.sum()) < float(err1.sum())


# ------------------------------------------------------------------------------------------------
# the precision-floor rule
# ------------------------------------------------------------------------------------------------
def test_fp32_floor_is_the_larger_of_the_restatement_error_and_one_rounding():
    want = torch.tensor([1.0, -8.0, 0.5], dtype=torch.float64)
    assert fp32_floor(want.clone(), want) == EPS32 * 8.0
    assert fp32_floor(want + torch.tensor([0.0, 0.0, 0.25]), want) == 0.25
    assert fp32_floor(want + torch.tensor([2.0 ** -30, 0.0, 0.0]), want) == EPS32 * 8.0          # below one rounding: the rounding holds


def test_check_against_floor_passes_at_the_bound_and_fails_just_above(capsys):
    want = torch.zeros(4, dtype=torch.float64)
    want[0] = 1.0
    floor32 = want.clone()
    floor32[1] = 0.125                                  # floor 0.125, bound MARGIN * 0.125 = 0.5: every figure exact in binary
    got = want.clone()
    got[2] = MARGIN * 0.125
    check_against_floor("at the bound", got, floor32, want)
    assert "at the bound: error 5.000e-01, bound 5.000e-01 (1.000)" in capsys.readouterr().out
    got[2] = MARGIN * 0.125 * (1 + 2.0 ** -40)
    with pytest.raises(AssertionError):
        check_against_floor("just above", got, floor32, want)
    check_against_floor("wider margin", got, floor32, want, margin=2 * MARGIN)


# ------------------------------------------------------------------------------------------------
# guard buffers
# ------------------------------------------------------------------------------------------------
def test_guarded_buffer_round_trips_and_catches_both_faults():
    dev = torch.device("cpu")
    buf, view = guarded(dev, 3, 5)
    assert view.shape == (3, 5) and buf.numel() == 15 + 64 and bool(torch.isnan(buf).all())
    data = randn(4, 3, 5)
    view.copy_(data)
    assert torch.equal(read_guarded(buf, view), data)
    buf[15] = 1.0                                       # one element past the view
    with pytest.raises(AssertionError, match="guard row"):
        read_guarded(buf, view)
    buf[15] = float("nan")
    view[2, 4] = float("nan")                           # one element never written
    with pytest.raises(AssertionError, match="unwritten"):
        read_guarded(buf, view)


# ------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------
def test_metrics_on_hand_computed_vectors():
    want, got = torch.tensor([3.0, 4.0]), torch.tensor([3.0, 1.0])          # difference (0, -3)
    assert rel_l2(got, want) == pytest.approx(3.0 / 5.0, rel=1e-12)
    assert rel_max(got, want) == pytest.approx(3.0 / 4.0, rel=1e-12)
    assert cosine(got, want) == pytest.approx(13.0 / (10.0 ** 0.5 * 5.0), rel=1e-12)
    assert rel_l2(want, want) == 0.0 and rel_max(want, want) == 0.0 and cosine(want, -want) == pytest.approx(-1.0, rel=1e-12)
