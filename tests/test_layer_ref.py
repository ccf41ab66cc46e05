"""CPU self-checks of tests/layer_ref.py: every case of tests/test_gpu_layer_ops.py holds the edge
it is there for in its reference values, so that no GPU case passes vacuously.  No GPU needed."""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import bits

NEG_ZERO = 0x80000000


def swiglu_shapes():
    out = [(t, k, max(fs), 1) for t, k, fs in R.DECODE_SWIGLU]
    out += [(t, k, R.GEN_F, max(R.N_GEN)) for t in (R.Q4_0, R.Q4_1) for k in R.GEN_K]
    out += [(t, k, R.BATCH_F, R.N_MAX) for t in R.ALL_TYPES for k in R.BATCH_K]
    return out


def resid_shapes():
    out = [(t, k, max(ms), 1) for t, _, k, ms in R.DECODE_RESID]
    out += [(t, k, R.GEN_M, max(R.N_GEN)) for t in (R.Q4_0, R.Q4_1) for k in R.GEN_K + [R.GEN_RESID_LONG[0]]]
    out += [(t, k, R.BATCH_M, R.N_MAX) for t in R.ALL_TYPES for k in R.BATCH_K]
    return out


def qkv_shapes():
    out = [(t, k, e, h, 1) for t, k, e, h in R.DECODE_QKV]
    out += [(t, k, R.GEN_E, R.GEN_H, max(R.N_GEN)) for t in (R.Q4_0, R.Q4_1) for k in R.GEN_K]
    out += [(t, k, R.BATCH_E, R.BATCH_H, R.N_MAX) for t in R.ALL_TYPES for k in R.BATCH_K]
    return out


def ids(shapes):
    return ["%s-%s" % (R.TYPE_NAME[s[0]], "-".join(str(v) for v in s[1:])) for s in shapes]


def check_u_edges(oracle, wtype, a1, a3, u, f):
    """both signs of zero in u, finite values, |a1| below the f16 maximum, a zero block of u"""
    assert np.all(np.isfinite(u)) and np.abs(a1).max() < 65504
    z = bits(u)
    assert np.any(z == 0) and np.any(z == NEG_ZERO)
    assert np.all(a1[:, R.ZERO_W1_ROW] == 0) and np.all(a3[:, R.ZERO_W3_ROW] == 0)
    assert np.all(u[:, R.ZERO_BLOCK] == 0) and np.any(u[:, :32] != 0)
    if R.is_q4(wtype):
        bb = R.BLOCK_BYTES[wtype]
        blk = oracle.quantize(np.ascontiguousarray(u[0, :f]), wtype).reshape(-1, bb)
        head = np.ascontiguousarray(blk[:2, :bb - 16]).view(np.float32)  # d (and m) of blocks 0 and 1
        assert np.all(head[1] == 0) and head[0, 0] != 0                  # the quantizers' id = 0 branch
    if a1.size >= 2000:
        # the silu table's ends: it flushes to zero below about -20.5 and is the identity far above
        assert a1.min() < -20.5 and a1.max() > 20.5
        tab = oracle.table_silu()
        h = R.f16_bits(oracle, np.array([a1.min(), a1.max()], np.float32))
        assert tab[h[0]] in (0x0000, 0x8000) and tab[h[1]] == h[1]


@pytest.mark.parametrize("shape", swiglu_shapes(), ids=ids(swiglu_shapes()))
def test_swiglu_cases_hold_their_edges(oracle, shape):
    wtype, k, f, n = shape
    c = R.swiglu_case(oracle, wtype, k, f, n)
    assert c["u"].shape == (n, f)
    check_u_edges(oracle, wtype, c["a1"], c["a3"], c["u"], f)


@pytest.mark.parametrize("shape", resid_shapes(), ids=ids(resid_shapes()))
def test_resid_cases_hold_their_edges(oracle, shape):
    wtype, k, m, n = shape
    c = R.resid_case(oracle, wtype, k, m, n)
    y0, dot, ref = c["y0"], c["dot"], c["ref"]
    assert ref.shape == (n, m) and np.all(np.isfinite(ref))
    assert np.all(bits(y0[:, 0]) == 0) and np.all(bits(y0[:, 1]) == NEG_ZERO) and np.all(bits(y0[:, 3]) == NEG_ZERO)
    assert np.all(y0[:, 2] == np.float32(1e30)) and np.all(y0[:, 4] == np.float32(1e-30))
    assert np.all(dot[:, 3] == 0)                                 # the zero weight row meets y = -0.0
    assert np.all(ref[:, 2] == y0[:, 2]) and np.all(ref[:, 0] == dot[:, 0])   # y far larger, y = 0
    assert np.all(bits(ref[:, 4]) == bits(dot[:, 4]))             # y far smaller than the dot
    # the add rounds: cells where the result is neither operand, and not their exact sum
    rounded = (ref != y0) & (ref != dot) & (ref.astype(np.float64) != dot.astype(np.float64) + y0.astype(np.float64))
    assert np.count_nonzero(rounded) >= 8
    assert len(np.unique(bits(ref[:, 5:]))) > ref[:, 5:].size // 2


@pytest.mark.parametrize("shape", qkv_shapes(), ids=ids(qkv_shapes()))
def test_qkv_cases_hold_their_edges(oracle, shape):
    wtype, k, E, H, n_max = shape
    c = R.qkv_case(oracle, wtype, k, E, H, n_max)
    assert np.all(np.isfinite(c["qkv"])) and np.all(c["qkv"][:, [E + 4, E + 5]] == 0)
    for n in sorted({1, n_max}):
        for n_past in R.n_past_set(n):
            q16, kc, vc = R.qkv_expected(oracle, c, n, n_past)
            K, K0 = kc.reshape(R.N_CTX, E), c["kc0"].reshape(R.N_CTX, E)
            V, V0 = vc.reshape(E, R.N_CTX), c["vc0"].reshape(E, R.N_CTX)
            rows = np.arange(n_past, n_past + n)
            other = np.setdiff1d(np.arange(R.N_CTX), rows)
            # a changed and an unchanged cell in each cache: the written positions, nothing else
            assert np.any(K[rows] != K0[rows]) and np.array_equal(K[other], K0[other])
            assert np.any(V[:, rows] != V0[:, rows]) and np.array_equal(V[:, other], V0[:, other])
            assert np.all((K[rows][:, 4:6] & 0x7FFF) == 0)        # RoPE of the zero pair: +-0
            assert np.any(q16 != 0)
    # position 0 leaves even elements as they are (a * 1 - b * 0), the last table row does not
    q0, _, _ = R.qkv_expected(oracle, c, 1, 0)
    ql, _, _ = R.qkv_expected(oracle, c, 1, R.N_CTX - 1)
    assert np.array_equal(q0[0], R.f16_bits(oracle, c["qkv"][0, :E])) and not np.array_equal(q0, ql)


@pytest.mark.parametrize("wtype", R.ALL_TYPES, ids=[R.TYPE_NAME[t] for t in R.ALL_TYPES])
def test_ffn_cases_hold_their_edges(oracle, wtype):
    c = R.ffn_case(oracle, wtype, R.FFN_K, R.FFN_F, R.N_MAX)
    s = R.swiglu_case(oracle, wtype, R.FFN_K, R.FFN_F, R.N_MAX)
    check_u_edges(oracle, wtype, s["a1"], s["a3"], c["u"], R.FFN_F)
    ref, x, dot = c["ref"], c["x"], c["dot"]
    assert ref.shape == (R.N_MAX, R.FFN_K) and np.all(np.isfinite(ref))
    assert np.count_nonzero((ref != x) & (ref != dot)) > ref.size // 2
    assert len({ref[t].tobytes() for t in range(R.N_MAX)}) == R.N_MAX       # every row differs


@pytest.mark.parametrize("n_embd", R.EMBED_E)
@pytest.mark.parametrize("wtype", R.ALL_TYPES, ids=[R.TYPE_NAME[t] for t in R.ALL_TYPES])
def test_embed_cases_hold_their_edges(oracle, wtype, n_embd):
    c = R.embed_case(oracle, wtype, n_embd)
    ref, tok = c["ref"], c["tokens"].tolist()
    assert tok == [0, 63, 5, 5, 17] and ref.shape == (5, n_embd) and np.all(np.isfinite(ref))
    assert np.array_equal(ref[2], ref[3]) and not np.array_equal(ref[0], ref[1])
    if R.is_q4(wtype):
        for i in (1, 2):                     # tokens 63 and 5: block 1 has d = 0
            assert len(np.unique(ref[i, 32:64])) == 1            # (q - 8) * 0, or 0 * q + m
            assert len(np.unique(ref[i, :32])) > 4
        assert len(np.unique(ref[0, 32:64])) > 4
