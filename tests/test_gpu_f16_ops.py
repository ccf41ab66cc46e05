"""The two f16 kernels (matvec_f16.hip, mm_f16.hip) against the oracle's ggml_vec_dot_f16.

Expected: y[t][r] = orc_vec_dot_f16(K, w16[r], f16(a[t])), a = x, or a = orc_rms_norm(x) * g
(multiplied in f32) with a norm weight; f32 -> f16 by numpy (RNE, like _cvtss_sh).  Compared
as uint32 bits.  The reference values are computed once per (K, g) and shared by the cases.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_MAX = 250          # not a multiple of 8: the row tail
N_MAX = 40
N_SPECIAL = 7        # rows 0..6 of the inputs, see inputs()
ROW_ZERO, ROW_SUBNORMAL, ROW_CANCEL = 3, 4, 5
K_DECODE = (256, 4096, 5120, 8192, 11008, 13824, 22016)
K_BATCH = (256, 4096, 11008)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def weights(K):
    """[M_MAX][K] f16 bits: N(0, 0.02) with -0 and f16 subnormals sprinkled in"""
    rng = np.random.default_rng(1000 + K)
    w = (rng.standard_normal((M_MAX, K)) * 0.02).astype(np.float16).view(np.uint16).copy()
    flat = w.reshape(-1)
    flat[::97] = 0x8000                                              # -0
    sub = rng.integers(1, 1024, size=flat[5::101].size).astype(np.uint16)
    sub |= (rng.integers(0, 2, size=sub.size).astype(np.uint16) << 15)
    flat[5::101] = sub                                               # +- subnormals
    assert np.isfinite(w.view(np.float16)).all()
    return w


def inputs(K):
    """[N_MAX][K] f32: magnitudes 1e-3, 1, 37 (as tests/golden/make_golden.py), a row of zeros, a
    row whose f16 images are subnormal, a cancelling row (alternating +-1024 with small values
    between), one more unit row, then the three magnitudes in turn.  All |x| < 65504."""
    rng = np.random.default_rng(2000 + K)
    x = np.zeros((N_MAX, K), np.float32)
    mags = (1e-3, 1.0, 37.0)
    for i, s in enumerate(mags):
        x[i] = rng.standard_normal(K) * s
    x[ROW_ZERO] = 0.0
    x[ROW_SUBNORMAL] = rng.uniform(1e-7, 6e-5, K) * rng.choice([-1.0, 1.0], K)
    c = rng.standard_normal(K) * 1e-3
    c[0::4] = 1024.0
    c[2::4] = -1024.0
    x[ROW_CANCEL] = c
    x[6] = rng.standard_normal(K)
    for i in range(N_SPECIAL, N_MAX):
        x[i] = rng.standard_normal(K) * mags[i % 3]
    x = np.clip(x, -60000.0, 60000.0).astype(np.float32)
    sub16 = x[ROW_SUBNORMAL].astype(np.float16).view(np.uint16)
    assert ((sub16 & 0x7c00) == 0).all() and (sub16 & 0x3ff).any()
    return x


class Case:
    """weights, inputs, norm weight and the oracle's expected rows for one K (built once)"""
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

    def act16(self, with_g):
        x = self.x[:self.rows]
        if with_g:
            y = np.zeros_like(x)
            self.oracle.lib.orc_rms_norm(np.ascontiguousarray(x), self.K, len(x), y)
            x = (y * self.g[None, :]).astype(np.float32)
        return np.ascontiguousarray(x.astype(np.float16).view(np.uint16))

    def expected(self, with_g):
        if with_g not in self._exp:
            a16 = self.act16(with_g)
            dot = self.oracle.lib.orc_vec_dot_f16
            out = np.zeros((self.rows, M_MAX), np.float32)
            for t in range(self.rows):
                for r in range(M_MAX):
                    out[t, r] = dot(self.K, self.w[r], a16[t])
            assert np.isfinite(out).all()
            self._exp[with_g] = out
        return self._exp[with_g]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("M", [8, 72, 250])
@pytest.mark.parametrize("K", K_DECODE)
def test_decode_matvec_vs_oracle(lvk, oracle, K, M, with_g):
    c = Case.get(oracle, K)
    exp = c.expected(with_g)
    for t in range(N_SPECIAL):
        y = lvk.mul_mat_f16(c.w[:M], c.x[t:t + 1], g=c.g if with_g else None, kernel=1)
        bad = np.flatnonzero(bits(y[0]) != bits(exp[t, :M]))
        assert bad.size == 0, "input row %d: %d of %d rows differ, first %s" % (t, bad.size, M, bad[:8])


@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("N", [2, 15, 16, 17, 40])
@pytest.mark.parametrize("M", [72, 250])
@pytest.mark.parametrize("K", K_BATCH)
def test_batched_matmul_vs_oracle(lvk, oracle, K, M, N, with_g):
    c = Case.get(oracle, K)
    exp = c.expected(with_g)
    y = lvk.mul_mat_f16(c.w[:M], c.x[:N], g=c.g if with_g else None, kernel=2)
    assert y.shape == (N, M)
    bad = np.argwhere(bits(y) != bits(exp[:N, :M]))
    assert bad.size == 0, "%d of %d values differ, first (token, row) %s" % (len(bad), N * M, bad[:8].tolist())


def test_auto_kernel_and_refusals(lvk, oracle):
    """kernel=0 picks the decode matvec for one row and the batched kernel beyond; any other
    combination is refused"""
    c = Case.get(oracle, 256)
    exp = c.expected(False)
    assert np.array_equal(bits(lvk.mul_mat_f16(c.w[:72], c.x[:1]))[0], bits(exp[0, :72]))
    assert np.array_equal(bits(lvk.mul_mat_f16(c.w[:72], c.x[:5])), bits(exp[:5, :72]))
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f16(c.w[:72], c.x[:2], kernel=1)        # the matvec takes one row
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f16(c.w[:72], c.x[:2], kernel=3)
    with pytest.raises(RuntimeError):
        lvk.mul_mat_f16(c.w[:72, :128], c.x[:2, :128])      # k % 256 != 0


@pytest.mark.parametrize("K", K_BATCH)
def test_cancelling_row_depends_on_order(oracle, K):
    """the cancelling input row cannot go soft: a plain float32 sum over k of the same f16
    products gives other bits than the reference's 32 chains for most weight rows"""
    c = Case.get(oracle, K)
    exp = c.expected(False)[ROW_CANCEL]
    a = c.act16(False)[ROW_CANCEL].view(np.float16).astype(np.float32)
    w = c.w.view(np.float16).astype(np.float32)
    plain = np.array([np.sum(w[r] * a, dtype=np.float32) for r in range(M_MAX)], np.float32)
    differ = int((bits(plain) != bits(exp)).sum())
    print("K %d: plain sum differs from the chains in %d of %d rows" % (K, differ, M_MAX))
    assert differ > M_MAX // 2
