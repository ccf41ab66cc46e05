"""The batched decode step's Q4_0 matmul at the 13B / 30B / 65B row lengths (matvec_cols_long.hip through
lvk_cols_store / _resid / _swiglu) against the CPU oracle: bit equality with tests/layer_ref.py.

Row lengths: 5120 (5 chunks: an odd stream, the padding position), 6656 (6 + 16 blocks), 8192 (8),
13824 / 17920 / 22016 (13 / 17 / 21 chunks + 16 blocks, the tiles of 16 / 12 / 10).  Columns n, with T
the row length's widest tile: 2, 5 (a partial tile), T, T + 1 (a second launch of one column) and 24
(tiled inside the workgroup where T < 12).  Rows: 72 (9 row groups, fewer than workgroups: the column
split), 2056 (257 groups: an uneven split) at n = 2 and T + 1, and once 18440 (2305 groups: a wave
takes two or three row groups, the ring runs across their boundary, with odd and even streams).  The
resid cases' y0 carries +-0, 1e30, 1e-30 and a zero weight row.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import Q4_0, bits

pytestmark = pytest.mark.gpu

TILE = {5120: 16, 6656: 16, 8192: 16, 13824: 16, 17920: 12, 22016: 10}
M_SMALL, M_BIG, M_CROSS = 72, 2056, 18440


def shapes(k):
    """(m, n) of row length k"""
    t = TILE[k]
    return [(M_SMALL, n) for n in (2, 5, t, t + 1, 24)] + [(M_BIG, n) for n in (2, t + 1)]


# (k, m, n) at the n_embd lengths; (input, k, m, n) with input 1 the Wo role, 0 the W2 role
EMBD = [(k, m, n) for k in (5120, 6656, 8192) for m, n in shapes(k)]
RESID = [(1, k, m, n) for k, m, n in EMBD] + [(0, k, m, n) for k in (13824, 17920, 22016) for m, n in shapes(k)]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def assert_rows_equal(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    d = np.argwhere(got != want)
    assert len(d) == 0, "%s: %d cells differ, the first at row %d, column %d" % (what, len(d), d[0][0], d[0][1])


def n_ref(m):
    """one reference per (k, m): the small matrix with every column count, the large one up to T + 1 = 17"""
    return 24 if m == M_SMALL else 17


@pytest.mark.parametrize("k,m,n", EMBD + [(5120, M_CROSS, 2)])
def test_cols_long_store(lvk, oracle, k, m, n):
    c = R.qkv_case(oracle, Q4_0, k, (m + 2) // 3, 1, 2 if m == M_CROSS else n_ref(m))    # w [>= m][k], the dots before RoPE
    got = lvk.cols_store(Q4_0, c["w"][:m], k, c["g"], c["x"][:n])
    assert_rows_equal(got, c["qkv"][:n, :m], "store k=%d m=%d n=%d" % (k, m, n))


@pytest.mark.parametrize("inp,k,m,n", RESID)
def test_cols_long_resid(lvk, oracle, inp, k, m, n):
    c = R.resid_case(oracle, Q4_0, k, m, n_ref(m))
    got = lvk.cols_resid(Q4_0, c["w"], k, c["a"][:n], c["y0"][:n], input=inp)
    assert_rows_equal(got, c["ref"][:n], "resid input=%d k=%d m=%d n=%d" % (inp, k, m, n))


@pytest.mark.parametrize("k,m,n", EMBD)
def test_cols_long_swiglu(lvk, oracle, k, m, n):
    f = m // 2                                      # the interleaved W1|W3 image has m rows
    c = R.swiglu_case(oracle, Q4_0, k, f, n_ref(m))
    got = lvk.cols_swiglu(Q4_0, c["w1"], c["w3"], k, c["g"], c["x"][:n])
    assert_rows_equal(got, c["u"][:n], "swiglu k=%d f=%d n=%d" % (k, f, n))


def test_refusals_then_a_valid_call(lvk, oracle):
    """what the entries keep refusing at the new row lengths (another weight type, one column, rows that are
    no multiple of 8, a null pointer, an n_ff length for store and swiglu), then a valid call that matches"""
    s = R.qkv_case(oracle, Q4_0, 5120, 24, 1, 24)
    r, g = R.resid_case(oracle, Q4_0, 5120, M_SMALL, 24), R.swiglu_case(oracle, Q4_0, 5120, M_SMALL // 2, 24)
    w, x, y0 = s["w"], s["x"][:2], r["y0"][:2]
    bad = [dict(wtype=t) for t in (R.Q4_1, R.F16, R.F32)] + [dict(n=1), dict(m=68), dict(w=None), dict(k=13824)]
    for b in bad:
        a = dict(dict(wtype=Q4_0, w=w, k=5120, n=2, m=72), **b)
        calls = [lambda: lvk.cols_store(a["wtype"], a["w"], a["k"], s["g"], x, n=a["n"], m=a["m"]),
                 lambda: lvk.cols_swiglu(a["wtype"], a["w"], g["w3"], a["k"], g["g"], x, n=a["n"], f=a["m"] // 2)]
        if "k" not in b:
            calls.append(lambda: lvk.cols_resid(a["wtype"], a["w"], a["k"], r["a"][:2], y0, n=a["n"], m=a["m"]))
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
    assert_rows_equal(lvk.cols_store(Q4_0, w, 5120, s["g"], x), s["qkv"][:2], "store after the refusals")
