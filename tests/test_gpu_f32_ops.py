"""The two f32 kernels (matvec_f32.hip, mm_f32.hip) against ggml_vec_dot_f32.

Expected: y[t][r] = ggml_vec_dot_f32(K, w[r], a[t]), a = x, or a = orc_rms_norm(x) * g
(multiplied in f32) with a norm weight, computed by the numpy restatement of the reference's
AVX2 dot (tests/f32_restatement.py, pinned by tests/test_f32_restatement.py).  Compared as
uint32 bits, no tolerance.  The expected values are computed once per (K, g) and shared by the
cases.
"""
import numpy as np
import pytest

from f32_restatement import M_MAX, N_MAX, N_SPECIAL, bits, dot_f32, inputs, weights

pytestmark = pytest.mark.gpu

# 256: below one chunk of loads in flight; 17920, 22016: more than 64 KiB of staged row
K_DECODE = (256, 4096, 5120, 11008, 13824, 17920, 22016)
K_BATCH = (256, 4096, 11008)


class Case:
    """weights, inputs, norm weight and the expected rows for one K (built once)"""
    _cache = {}

    def __init__(self, oracle, K, rows):
        self.K, self.rows = K, rows
        self.w = weights(K)
        self.x = inputs(K)
        self.g = (1.0 + 0.1 * np.random.default_rng(3000 + K).standard_normal(K)).astype(np.float32)
        self.oracle = oracle
        self._exp = {}

    @classmethod
    def get(cls, oracle, K):
        if K not in cls._cache:
            cls._cache[K] = Case(oracle, K, N_MAX if K in K_BATCH else N_SPECIAL)
        return cls._cache[K]

    def act(self, with_g):
        x = self.x[:self.rows]
        if with_g:
            y = np.zeros_like(x)
            self.oracle.lib.orc_rms_norm(np.ascontiguousarray(x), self.K, len(x), y)
            x = (y * self.g[None, :]).astype(np.float32)
        return np.ascontiguousarray(x)

    def expected(self, with_g):
        if with_g not in self._exp:
            out = dot_f32(self.w, self.act(with_g))
            assert out.shape == (self.rows, M_MAX) and np.isfinite(out).all()
            self._exp[with_g] = out
        return self._exp[with_g]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("M", [8, 72, 250])
@pytest.mark.parametrize("K", K_DECODE)
def test_decode_matvec_vs_restatement(lvk, oracle, K, M, with_g):
    c = Case.get(oracle, K)
    exp = c.expected(with_g)
    for t in range(N_SPECIAL):
        y = lvk.mul_mat_f32(c.w[:M], c.x[t:t + 1], g=c.g if with_g else None, kernel=1)
        bad = np.flatnonzero(bits(y[0]) != bits(exp[t, :M]))
        assert bad.size == 0, "input row %d: %d of %d rows differ, first %s" % (t, bad.size, M, bad[:8])


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("N", [2, 15, 16, 17, 40])
@pytest.mark.parametrize("M", [8, 72, 250])
@pytest.mark.parametrize("K", K_BATCH)
def test_batched_matmul_vs_restatement(lvk, oracle, K, M, N, with_g):
    """M 8 is half a 16-row tile, 72 four and a half, 250 leaves a tail of 10 rows; N 15 / 16 /
    17 straddle the 16-token tile"""
    c = Case.get(oracle, K)
    exp = c.expected(with_g)
    y = lvk.mul_mat_f32(c.w[:M], c.x[:N], g=c.g if with_g else None, kernel=2)
    assert y.shape == (N, M)
    bad = np.argwhere(bits(y) != bits(exp[:N, :M]))
    assert bad.size == 0, "%d of %d values differ, first (token, row) %s" % (len(bad), N * M, bad[:8].tolist())


def test_auto_kernel_and_refusals(lvk, oracle):
    """kernel=0 picks the decode matvec for one row and the batched kernel beyond; any other
    combination is refused"""
    c = Case.get(oracle, 256)
    exp = c.expected(False)
    assert np.array_equal(bits(lvk.mul_mat_f32(c.w[:72], c.x[:1]))[0], bits(exp[0, :72]))
    assert np.array_equal(bits(lvk.mul_mat_f32(c.w[:72], c.x[:5])), bits(exp[:5, :72]))
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f32(c.w[:72], c.x[:2], kernel=1)        # the matvec takes one row
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f32(c.w[:72], c.x[:2], kernel=3)
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f32(c.w[:72, :128], c.x[:2, :128])      # k % 256 != 0
