"""The batched decode step's matmul (matvec_cols.hip through lvk_cols_store / _resid / _swiglu) against
the CPU oracle: bit equality with the expected values of tests/layer_ref.py.

Columns n: 2 (the smallest tile), 5 (a partial tile of 8), 16 (a full tile), 17 and 33 (whole tiles of
16 tiled inside the workgroup, then a second launch of one column).  Rows: 72 (9 row groups, fewer
than workgroups), 4104 (513 groups: an uneven split, a wave's second group behind the ring's
cross-group prefetch), f = 11012 (row groups that the compute units do not divide).  K = 11008 ends in
a partial chunk of 24 blocks.  The resid cases' y0 carries +-0, 1e30, 1e-30 and a zero weight row.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import Q4_0, bits

pytestmark = pytest.mark.gpu

N_COLS = [2, 5, 16, 17, 33]
N_MAX = 33
N_LONG = [2, 17]            # the column counts of the large K = 11008 / f = 11012 cases
# (input, k, m, n): input 1 the Wo role, input 0 the W2 role
RESID = ([(1, 4096, m, n) for m in (72, 4104) for n in N_COLS] + [(0, 11008, 72, n) for n in N_COLS] +
         [(0, 11008, 4104, n) for n in N_LONG])
SWIGLU = [(288, n) for n in N_COLS] + [(11012, n) for n in N_LONG]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def assert_rows_equal(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    d = np.argwhere(got != want)
    assert len(d) == 0, "%s: %d cells differ, the first at row %d, column %d" % (what, len(d), d[0][0], d[0][1])


def store_case(oracle):
    return R.qkv_case(oracle, Q4_0, 4096, 1368, 1, N_MAX)        # w [4104][4096], the dots before RoPE


def resid_case(oracle, k, m):
    return R.resid_case(oracle, Q4_0, k, m, N_MAX if (k, m) != (11008, 4104) else max(N_LONG))


@pytest.mark.parametrize("n", N_COLS)
@pytest.mark.parametrize("m", [72, 4104])
def test_cols_store(lvk, oracle, m, n):
    c = store_case(oracle)
    got = lvk.cols_store(Q4_0, c["w"][:m], 4096, c["g"], c["x"][:n])
    assert_rows_equal(got, c["qkv"][:n, :m], "store m=%d n=%d" % (m, n))


@pytest.mark.parametrize("inp,k,m,n", RESID)
def test_cols_resid(lvk, oracle, inp, k, m, n):
    c = resid_case(oracle, k, m)
    got = lvk.cols_resid(Q4_0, c["w"][:m], k, c["a"][:n], c["y0"][:n, :m], input=inp)
    assert_rows_equal(got, c["ref"][:n, :m], "resid input=%d k=%d m=%d n=%d" % (inp, k, m, n))


@pytest.mark.parametrize("f,n", SWIGLU)
def test_cols_swiglu(lvk, oracle, f, n):
    c = R.swiglu_case(oracle, Q4_0, 4096, f, N_MAX if f == 288 else max(N_LONG))
    got = lvk.cols_swiglu(Q4_0, c["w1"][:f], c["w3"][:f], 4096, c["g"], c["x"][:n])
    assert_rows_equal(got, c["u"][:n, :f], "swiglu f=%d n=%d" % (f, n))


def test_refusals_then_a_valid_call(lvk, oracle):
    """what the three entries refuse (another weight type, a row length that is not compiled in, one
    column, rows that are no multiple of 8, a null pointer), then a valid call that still matches"""
    s, r, g = store_case(oracle), resid_case(oracle, 4096, 72), R.swiglu_case(oracle, Q4_0, 4096, 288, N_MAX)
    w, x, y0 = s["w"][:72], s["x"][:2], r["y0"][:2, :72]
    bad = [dict(wtype=t) for t in (R.Q4_1, R.F16, R.F32)] + [dict(k=256), dict(n=1), dict(m=68), dict(w=None)]
    for b in bad:
        a = dict(dict(wtype=Q4_0, w=w, k=4096, n=2, m=72), **b)
        calls = [lambda: lvk.cols_store(a["wtype"], a["w"], a["k"], s["g"], x, n=a["n"], m=a["m"]),
                 lambda: lvk.cols_resid(a["wtype"], a["w"], a["k"], r["a"][:2], y0, n=a["n"], m=a["m"]),
                 lambda: lvk.cols_swiglu(a["wtype"], a["w"], g["w3"][:72], a["k"], g["g"], x, n=a["n"], f=a["m"] // 2)]
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
    assert_rows_equal(lvk.cols_store(Q4_0, w, 4096, s["g"], x), s["qkv"][:2, :72], "store after the refusals")
