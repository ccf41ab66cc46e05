"""numpy restatement of the reference's ggml_vec_dot_f32 (AVX2, ggml.c:1713-1748), the expected
values of the f32 kernels' tests (pinned on the CPU by tests/test_f32_restatement.py).

fma32 is an exact vectorised fmaf: the product of two float32 is exact in float64; the sum with
c is rounded to odd (TwoSum residual e; when e != 0 and the float64 significand is even, one
ulp toward e), so the final cast to float32 rounds the exact value once.  dot_f32 runs the 32
chains (accumulator a, lane l takes elements 32 st + 8 a + l in step order) and
GGML_F32x8_REDUCE: (s0+s1)+(s2+s3) per lane, S[l]+S[l+4], (t0+t1)+(t2+t3).
"""
import numpy as np


def fma32(a, b, c):
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def reduce32(acc):
    """[..., 32] chain values -> [...] (GGML_F32x8_REDUCE)"""
    s = acc.reshape(acc.shape[:-1] + (4, 8))
    a = (s[..., 0, :] + s[..., 1, :]) + (s[..., 2, :] + s[..., 3, :])
    t = a[..., :4] + a[..., 4:]
    return (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])


def dot_f32(w, x, step=fma32):
    """w [M][K], x [N][K] float32 -> [N][M] float32; step(w, x, acc) advances the chains"""
    w = np.ascontiguousarray(w, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    M, K = w.shape
    N = x.shape[0]
    assert K % 32 == 0 and x.shape[1] == K
    acc = np.zeros((N, M, 32), np.float32)
    for st in range(K // 32):
        acc = step(np.broadcast_to(w[None, :, 32 * st:32 * st + 32], acc.shape),
                   np.broadcast_to(x[:, None, 32 * st:32 * st + 32], acc.shape), acc)
    return reduce32(acc)


def unfused_step(w, x, acc):
    """acc + w * x with the product rounded to float32 first (what a missing fma would give)"""
    return acc + w * x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


M_MAX = 250          # not a multiple of 8 or 16: the row tails
N_MAX = 40
N_SPECIAL = 7        # rows 0..6 of inputs()
ROW_ZERO, ROW_SUBNORMAL, ROW_CANCEL = 3, 4, 5
UNIT_ROWS = (1, 6)


def weights(K):
    """[M_MAX][K] f32: N(0, 0.02) at full f32 precision with -0 and f32 subnormals sprinkled in"""
    rng = np.random.default_rng(1000 + K)
    w = (rng.standard_normal((M_MAX, K)) * 0.02).astype(np.float32)
    flat = w.reshape(-1).view(np.uint32)
    flat[::97] = 0x80000000                                          # -0
    sub = rng.integers(1, 1 << 23, size=flat[5::101].size).astype(np.uint32)
    sub |= rng.integers(0, 2, size=sub.size).astype(np.uint32) << 31
    flat[5::101] = sub                                               # +- subnormals
    assert np.isfinite(w).all()
    return w


def inputs(K):
    """[N_MAX][K] f32: magnitudes 1e-3, 1, 37, a row of zeros, a row of f32 subnormals, a
    cancelling row (alternating +-1024 with small values between), one more unit row, then the
    three magnitudes in turn"""
    rng = np.random.default_rng(2000 + K)
    x = np.zeros((N_MAX, K), np.float32)
    mags = (1e-3, 1.0, 37.0)
    for i, s in enumerate(mags):
        x[i] = rng.standard_normal(K) * s
    x[ROW_ZERO] = 0.0
    sub = rng.integers(1, 1 << 23, size=K).astype(np.uint32) | rng.integers(0, 2, size=K).astype(np.uint32) << 31
    x[ROW_SUBNORMAL] = sub.view(np.float32)
    c = rng.standard_normal(K) * 1e-3
    c[0::4] = 1024.0
    c[2::4] = -1024.0
    x[ROW_CANCEL] = c
    x[6] = rng.standard_normal(K)
    for i in range(N_SPECIAL, N_MAX):
        x[i] = rng.standard_normal(K) * mags[i % 3]
    assert np.isfinite(x).all()
    return x
