"""tests/util.py::assert_gemm_close on the CPU: a NaN compares false with every bound, so the helper checks the class of each output (finite,
NaN, +inf, -inf) against the correctly rounded exact value before it looks at distances.  The oracle's correctly rounded result passes; the
same result with one element replaced by a value of another class fails, wherever the element sits."""
import numpy as np
import pytest

from oracle import awq_ref
from sglang_awq_amd import synth
from tests.util import assert_gemm_close

M, K, N, G = 5, 64, 24, 32
OVER = {"f16": 1.0e6, "bf16": 1.0e39, "f32": 1.0e39}            # finite in float64, rounds to inf in the storage dtype
INF_AT, NEG_AT = (3, 7), (4, 2)


def _case(dt):
    qw, s, qz = synth.make_awq_weights(K, N, G, dt, "A", seed=7)
    x = synth.make_activations(M, K, dt, "A", seed=8)
    exact = awq_ref.awq_gemm_exact(x, qw, s, qz)
    exact[INF_AT] = OVER[dt]
    exact[NEG_AT] = -OVER[dt]
    with np.errstate(over="ignore"):
        y = awq_ref.from_f64(exact, dt)
    assert np.isposinf(awq_ref.to_f64(y, dt)[INF_AT]) and np.isneginf(awq_ref.to_f64(y, dt)[NEG_AT])
    return y, exact


def _put(y, at, value, dt):
    y = y.copy()
    y[at] = awq_ref.from_f64(np.array([value], dtype=np.float64), dt)[0]
    return y


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_correctly_rounded_result_passes(dt):
    y, exact = _case(dt)
    assert_gemm_close(y, exact, dt, atol=0.0 if dt != "f32" else 1e-3, what=dt)


# (where, value): NaN and +inf on a finite element (first, middle, last); the sign of an inf flipped, both ways; a finite value — the
# largest one, what a saturating conversion leaves — and a NaN where the rounded exact value is inf
POISON = [((0, 0), np.nan), ((2, 11), np.nan), ((M - 1, N - 1), np.nan), ((0, 0), np.inf), ((M - 1, N - 1), -np.inf),
          (INF_AT, -np.inf), (NEG_AT, np.inf), (INF_AT, 65504.0), (INF_AT, 0.0), (NEG_AT, -65504.0), (INF_AT, np.nan)]


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("at,value", POISON)
def test_one_element_of_another_class_fails(dt, at, value):
    y, exact = _case(dt)
    with pytest.raises(AssertionError):
        assert_gemm_close(_put(y, at, value, dt), exact, dt, what=dt)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_exact_nan_and_inf_need_the_same_class(dt):
    """An exact value that is itself NaN or inf (a poisoned input) wants NaN or the same inf, nothing else."""
    y, exact = _case(dt)
    exact[0, 0], exact[1, 1] = np.nan, -np.inf
    y = _put(_put(y, (0, 0), np.nan, dt), (1, 1), -np.inf, dt)
    assert_gemm_close(y, exact, dt, what=dt)
    for at, value in (((0, 0), 1.0), ((0, 0), np.inf), ((1, 1), np.nan), ((1, 1), np.inf), ((1, 1), -1.0)):
        with pytest.raises(AssertionError):
            assert_gemm_close(_put(y, at, value, dt), exact, dt, what=dt)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_finite_rules_are_unchanged(dt):
    """One finite element a whole ulp off still fails on the bound; 2 % of the elements on the neighbouring value still fail on the share."""
    y, exact = _case(dt)
    v = awq_ref.to_f64(y, dt)
    step = 2.0 ** (np.floor(np.log2(np.abs(v[1, 1]))) - {"f16": 10, "bf16": 7}[dt])
    with pytest.raises(AssertionError, match="elements off"):
        assert_gemm_close(_put(y, (1, 1), v[1, 1] + 4 * step, dt), exact, dt, atol=0.0, what=dt)
    z = y.copy()
    for i in range(3):                                           # 3 of 120: 2.5 %
        z[i, i] = awq_ref.from_f64(np.array([v[i, i] + 2.0 ** (np.floor(np.log2(np.abs(v[i, i]))) - {"f16": 10, "bf16": 7}[dt])]), dt)[0]
    with pytest.raises(AssertionError, match="differ from the correctly rounded"):
        assert_gemm_close(z, exact, dt, atol=1.0, what=dt)
