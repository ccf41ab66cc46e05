"""The numpy restatement of ggml_vec_dot_f32 (tests/f32_restatement.py), which the f32 GPU
tests take their expected bits from, pinned on the CPU: its fmaf against glibc's, its chains and
reduce against the oracle's ggml_vec_dot_f16 on data where both dots are the same function,
and a guard that the test data tells a fused chain from anything else."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from f32_restatement import (M_MAX, UNIT_ROWS, bits, dot_f32, fma32, inputs, unfused_step, weights)


@pytest.fixture(scope="module")
def fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    return lambda a, b, c: np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], np.float32)


def test_constructed_double_rounding_case(fmaf):
    """a = 1 + 2^-23, b = 64 (1 - 2^-23), c = 2^30 + 2^7: fmaf gives c; a float64 sum rounded to
    float32 gives c + 2^7"""
    a = np.array([1 + 2.0 ** -23], np.float32)
    b = np.array([64 * (1 - 2.0 ** -23)], np.float32)
    c = np.array([2.0 ** 30 + 2.0 ** 7], np.float32)
    want = fmaf(a, b, c)
    assert want[0] == c[0]
    assert np.array_equal(bits(fma32(a, b, c)), bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert naive[0] == c[0] + np.float32(2.0 ** 7)


def test_fma32_equals_libm_normal_range(fmaf):
    rng = np.random.default_rng(0)
    n = 4000
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1, 1e4], n)).astype(np.float32)
    # products near half an ulp of c: the cases a double-rounded sum gets wrong
    a[:1000] = (1 + rng.integers(0, 2 ** 23, 1000) * 2.0 ** -23).astype(np.float32)
    b[:500] = np.float32(0.5)
    b[500:1000] = np.float32(0.5 + 2.0 ** -24)
    c[:1000] = (2.0 ** 24 + 2 * rng.integers(0, 1000, 1000)).astype(np.float32)
    assert np.array_equal(bits(fma32(a, b, c)), bits(fmaf(a, b, c)))


def test_fma32_equals_libm_subnormal_results(fmaf):
    rng = np.random.default_rng(1)
    n = 2000
    a = (rng.standard_normal(n) * 1e-22).astype(np.float32)
    b = (rng.standard_normal(n) * 1e-20).astype(np.float32)
    c = rng.integers(1, 2 ** 23, n).astype(np.uint32).view(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    a[n // 2:] = (rng.standard_normal(n // 2) * 1e-19).astype(np.float32)     # products of the size of c
    want = fmaf(a, b, c)
    assert int(((np.abs(want) < 1.17e-38) & (want != 0)).sum()) > n // 2
    assert np.array_equal(bits(fma32(a, b, c)), bits(want))


@pytest.mark.parametrize("K", [256, 4096, 11008])
def test_restatement_equals_oracle_f16_dot_on_f16_data(oracle, K):
    """on f16-representable operands both conversions of ggml_vec_dot_f16 are exact, so it is
    ggml_vec_dot_f32 of the same values"""
    rng = np.random.default_rng(10 + K)
    w16 = (rng.standard_normal((24, K)) * 0.02).astype(np.float16)
    x16 = (rng.standard_normal((3, K)) * np.array([[1e-3], [1], [37]])).astype(np.float16)
    x16[1, 0::4] = 1024
    x16[1, 2::4] = -1024
    got = dot_f32(w16.astype(np.float32), x16.astype(np.float32))
    dot = oracle.lib.orc_vec_dot_f16
    wu, xu = np.ascontiguousarray(w16.view(np.uint16)), np.ascontiguousarray(x16.view(np.uint16))
    want = np.array([[dot(K, wu[r], xu[t]) for r in range(24)] for t in range(3)], np.float32)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("K", [256, 4096, 11008])
def test_data_cannot_go_soft(K):
    """on the unit-magnitude input rows an unfused acc + w x and a plain float32 sum each give
    other bits than the fused chains for more than half of the weight rows (measured 0.60-0.84
    and 0.73-0.92)"""
    w = weights(K)
    x = inputs(K)[list(UNIT_ROWS)]
    y = dot_f32(w, x)
    u = dot_f32(w, x, step=unfused_step)
    plain = np.stack([np.array([np.sum(w[r] * x[t], dtype=np.float32) for r in range(M_MAX)], np.float32)
                      for t in range(len(x))])
    for t in range(len(x)):
        du = int((bits(u[t]) != bits(y[t])).sum())
        dp = int((bits(plain[t]) != bits(y[t])).sum())
        print("K %d row %d: unfused differs in %d, plain sum in %d of %d rows" % (K, UNIT_ROWS[t], du, dp, M_MAX))
        assert du > M_MAX // 2 and dp > M_MAX // 2
