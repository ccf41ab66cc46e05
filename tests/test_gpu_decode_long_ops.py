"""The single-token Q4_0 decode kernel of the LLaMA 13B / 30B row lengths (matvec_cu_long.hip: K 5120 /
13824, 6656 / 17920) in every role of a layer, through path 1 (launch_matvec_cu) of the layer operators
and through the matmul operators, bit for bit against the CPU oracle (tests/layer_ref.py's cases).

The shapes per role, on 256 compute units: 72 rows (9 row groups: fewer than workgroups), the model's
size, and one row group more (some waves own one row group more than others).  QKV at n_embd 8192 is 12
row groups per workgroup on 8 waves: the ring crosses row groups on an odd chunk count (5).  The 30B
lengths and 13824 end in a 16-block chunk; 5 x 1 and 7 x 1 chunk streams end on the padding position.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import Q4_0, bits
from test_gpu_layer_ops import assert_rows_equal, check_qkv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.mark.parametrize("k,E,H", [(5120, 1024, 8), (5120, 5120, 40), (5120, 8192, 64), (6656, 1024, 8), (6656, 6656, 52)])
def test_qkv(lvk, oracle, k, E, H):
    """PRO_NORM + EPI_QKV: RoPE at positions 0, 7 and n_ctx - 1, the q16 row, the K row, the V column"""
    c = R.qkv_case(oracle, Q4_0, k, E, H, 1)
    check_qkv(lvk, oracle, c, 1, 1, 1, "launch_matvec_cu EPI_QKV q4_0 k=%d n_embd=%d" % (k, E))


@pytest.mark.parametrize("k,f,f_max", [(5120, 288, 13828), (5120, 13824, 13828), (5120, 13828, 13828),
                                       (6656, 288, 17920), (6656, 17920, 17920)])
def test_swiglu(lvk, oracle, k, f, f_max):
    """PRO_NORM + EPI_SWIGLU_F32 on the interleave-by-4 W1|W3 image"""
    c = R.swiglu_case(oracle, Q4_0, k, f_max, 1)
    u = lvk.layer_swiglu(Q4_0, 1, c["w1"][:f], c["w3"][:f], k, c["g"], c["x"], want="u")
    assert_rows_equal(u, c["u"][:, :f], "launch_matvec_cu EPI_SWIGLU_F32 q4_0 k=%d f=%d" % (k, f))


RESID = [(inp, k, m, e + 8) for inp, k, e in [(1, 5120, 5120), (1, 6656, 6656), (0, 13824, 5120), (0, 17920, 6656)]
         for m in (72, e, e + 8)]


@pytest.mark.parametrize("inp,k,m,m_max", RESID, ids=["in%d-k%d-m%d" % t[:3] for t in RESID])
def test_resid(lvk, oracle, inp, k, m, m_max):
    """EPI_RESID: PRO_ACTQ (Wo, input 1) and PRO_ACTF (W2, input 0)"""
    c = R.resid_case(oracle, Q4_0, k, m_max, 1)
    y = lvk.layer_resid(Q4_0, 1, c["w"][:m], k, c["a"], c["y0"][:, :m], input=inp)
    assert_rows_equal(y, c["ref"][:, :m], "launch_matvec_cu EPI_RESID q4_0 input=%d k=%d m=%d" % (inp, k, m))


@pytest.mark.parametrize("m,k", [(72, 5120), (32000, 5120), (72, 6656), (72, 13824), (72, 17920)])
def test_mul_mat_pairs(lvk, oracle, m, k):
    """lm_head (PRO_NORM + EPI_STORE) and the plain operator (PRO_ACTF + EPI_STORE), n = 1"""
    rng = np.random.default_rng(m + 3 * k)
    w = R.make_weights(rng, Q4_0, m, k)
    x = (rng.standard_normal((1, k)) * 2.0).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    want = R.dots(oracle, Q4_0, w, R.convert(oracle, Q4_0, R.norm_rows(oracle, x, g)), k)
    assert_rows_equal(lvk.mul_mat_q_norm(Q4_0, w, m, k, g, x), want, "mul_mat_q_norm m=%d k=%d" % (m, k))
    want = R.dots(oracle, Q4_0, w, R.convert(oracle, Q4_0, x), k)
    assert_rows_equal(lvk.mul_mat_q(Q4_0, w, m, k, x), want, "mul_mat_q m=%d k=%d" % (m, k))


def test_refuses_a_pair_it_has_not(lvk, oracle):
    """PRO_NORM + EPI_QKV at k = 13824 has no instantiation: refused on the host ahead of any launch.  The
    entry point is called on the test's own buffers: it fails, the q16 row and both caches keep their
    bits, and a good call afterwards still matches"""
    E, H, k = 256, 2, 13824
    bad = R.qkv_case(oracle, Q4_0, k, E, H, 1)
    p = lambda a: a.ctypes.data
    w = np.ascontiguousarray(bad["w"])
    kc, vc, q16 = bad["kc0"].copy(), bad["vc0"].copy(), np.full(E, 0xA5A5, np.uint16)
    rc = lvk.lib.lvk_layer_qkv(Q4_0, 1, p(w), E, H, k, p(bad["g"]), p(bad["x"]), 1, R.N_CTX, 7, 1, p(kc), p(vc), p(q16))
    assert rc != 0
    assert np.array_equal(kc, bad["kc0"]) and np.array_equal(vc, bad["vc0"]) and (q16 == 0xA5A5).all()
    c = R.resid_case(oracle, Q4_0, k, 72, 1)
    y = lvk.layer_resid(Q4_0, 1, c["w"], k, c["a"], c["y0"], input=0)
    assert np.array_equal(bits(y), bits(c["ref"]))
