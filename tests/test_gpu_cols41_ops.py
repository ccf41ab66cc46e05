"""The batched decode step's Q4_1 matmul (matvec_cols41.hip through lvk_cols41_store / _resid / _swiglu)
against the CPU oracle: bit equality with the expected values of tests/layer_ref.py.

Row lengths: 5120 (5 chunks: the ring's slot flips between row groups), 13824 (13 chunks + 16 blocks,
the tile of 8), 11008 (a 24-block partial chunk, the tile of 12), 4096 once per entry.  Columns n, with
T the widest tile of the row length (16, 16, 12, 8): 2 (the smallest tile), 5 (a partial tile), T, and
T + 1 and 2T + 1 (whole tiles tiled inside the workgroup, then a second launch of one column).  Rows:
72 (9 row groups, fewer than workgroups), 4104 (513 groups: an uneven split, a wave's second group
behind the cross-group prefetch), f = 11012 (row groups that the compute units do not divide).  The
resid cases' y0 carries +-0, 1e30, 1e-30 and a zero weight row.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import Q4_1, bits

pytestmark = pytest.mark.gpu

N16 = [2, 5, 16, 17, 33]    # K = 4096 / 5120: T = 16
N8 = [2, 5, 8, 9, 17]       # K = 13824: T = 8
# (k, m, n)
STORE = [(5120, m, n) for m in (72, 4104) for n in N16] + [(4096, 72, 17)]
# (input, k, m, n): input 1 the Wo role, input 0 the W2 role; the large cases take the smallest and one tiled count
RESID = ([(1, 5120, m, n) for m in (72, 4104) for n in N16] + [(0, 13824, 72, n) for n in N8] +
         [(0, 13824, 4104, n) for n in (2, 9)] + [(0, 11008, 72, 13), (1, 4096, 72, 17)])
# (k, f, n)
SWIGLU = [(5120, 288, n) for n in N16] + [(5120, 11012, n) for n in (2, 17)] + [(4096, 288, 17)]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def n_max(cases, *key):
    """the most columns any case of this (k, m) takes: one reference per (k, m)"""
    return max(c[-1] for c in cases if tuple(c[-1 - len(key):-1]) == key)


def assert_rows_equal(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    d = np.argwhere(got != want)
    assert len(d) == 0, "%s: %d cells differ, the first at row %d, column %d" % (what, len(d), d[0][0], d[0][1])


def store_case(oracle, k, m):
    return R.qkv_case(oracle, Q4_1, k, m // 3, 1, n_max(STORE, k, m))       # w [m][k], the dots before RoPE


def resid_case(oracle, k, m):
    return R.resid_case(oracle, Q4_1, k, m, n_max(RESID, k, m))


def swiglu_case(oracle, k, f):
    return R.swiglu_case(oracle, Q4_1, k, f, n_max(SWIGLU, k, f))


@pytest.mark.parametrize("k,m,n", STORE)
def test_cols41_store(lvk, oracle, k, m, n):
    c = store_case(oracle, k, m)
    got = lvk.cols41_store(c["w"], k, c["g"], c["x"][:n])
    assert_rows_equal(got, c["qkv"][:n], "store k=%d m=%d n=%d" % (k, m, n))


@pytest.mark.parametrize("inp,k,m,n", RESID)
def test_cols41_resid(lvk, oracle, inp, k, m, n):
    c = resid_case(oracle, k, m)
    got = lvk.cols41_resid(c["w"], k, c["a"][:n], c["y0"][:n], input=inp)
    assert_rows_equal(got, c["ref"][:n], "resid input=%d k=%d m=%d n=%d" % (inp, k, m, n))


@pytest.mark.parametrize("k,f,n", SWIGLU)
def test_cols41_swiglu(lvk, oracle, k, f, n):
    c = swiglu_case(oracle, k, f)
    got = lvk.cols41_swiglu(c["w1"], c["w3"], k, c["g"], c["x"][:n])
    assert_rows_equal(got, c["u"][:n], "swiglu k=%d f=%d n=%d" % (k, f, n))


def test_refusals_then_a_valid_call(lvk, oracle):
    """what the three entries refuse (one column, a row length that is not compiled in, rows that are no
    multiple of 8, a null pointer, the Wo role at an n_ff row length), then a valid call that still matches"""
    s, r, g = store_case(oracle, 4096, 72), resid_case(oracle, 4096, 72), swiglu_case(oracle, 4096, 288)
    w, x, y0 = s["w"], s["x"][:2], r["y0"][:2]
    for b in [dict(n=1), dict(k=256), dict(m=68), dict(w=None)]:
        a = dict(dict(w=w, k=4096, n=2, m=72), **b)
        calls = [lambda: lvk.cols41_store(a["w"], a["k"], s["g"], x, n=a["n"], m=a["m"]),
                 lambda: lvk.cols41_resid(a["w"], a["k"], r["a"][:2], y0, input=1, n=a["n"], m=a["m"]),
                 lambda: lvk.cols41_swiglu(a["w"], g["w3"][:72], a["k"], g["g"], x, n=a["n"], f=a["m"] // 2)]
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
    with pytest.raises(RuntimeError):
        lvk.cols41_resid(w, 13824, np.zeros((2, 13824), np.float32), y0, input=1, n=2, m=72)
    assert_rows_equal(lvk.cols41_store(w, 4096, s["g"], x), s["qkv"][:2], "store after the refusals")
