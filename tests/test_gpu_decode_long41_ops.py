"""The single-token Q4_1 decode kernel of the LLaMA 30B / 65B row lengths (matvec_cu41_long.hip: K 6656 /
17920, 8192 / 22016) in every role of a layer, through path 1 (launch_matvec_cu) of the layer operators
and through the matmul operators, bit for bit against the CPU oracle (tests/layer_ref.py's cases).

The shapes per role, on 256 compute units: 72 rows (9 row groups, fewer than workgroups: every workgroup
has waves without a row group), the model's size, and one row group more (some waves own one row group
more than others).  Which case reaches which branch of the chunk stream:
  the padding position (7 chunks x 1 row group): every 72-row case at 6656, QKV at n_embd 1024 and f 288;
  the 16-block tail chunk: 6656, 17920, 22016; the whole-chunk row: 8192;
  a wave crossing row groups on an odd chunk count: QKV (9.75 row groups per workgroup on 8 waves) and
  W1|W3 (17.5) at 6656 in the model's size, the 32000-row lm_head;
  the same on an even chunk count: QKV (12) and W1|W3 (21.5) at 8192.  Wo and W2 have 3.25 / 4 row groups
  per workgroup on 4 / 8 waves, so no wave of theirs owns two: their model sizes cover workgroups with 3
  and 4 busy waves and the 18- and 22-chunk streams.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import Q4_1, bits
from test_gpu_layer_ops import assert_rows_equal, check_qkv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.mark.parametrize("k,E,H", [(6656, 1024, 8), (6656, 6656, 52), (8192, 1024, 8), (8192, 8192, 64)])
def test_qkv(lvk, oracle, k, E, H):
    """PRO_NORM + EPI_QKV: RoPE at positions 0, 7 and n_ctx - 1, the q16 row, the K row, the V column"""
    c = R.qkv_case(oracle, Q4_1, k, E, H, 1)
    check_qkv(lvk, oracle, c, 1, 1, 1, "launch_matvec_cu EPI_QKV q4_1 k=%d n_embd=%d" % (k, E))


@pytest.mark.parametrize("k,f,f_max", [(6656, 288, 17920), (6656, 17920, 17920), (8192, 288, 22016), (8192, 22016, 22016)])
def test_swiglu(lvk, oracle, k, f, f_max):
    """PRO_NORM + EPI_SWIGLU_F32 on the interleave-by-4 W1|W3 image"""
    c = R.swiglu_case(oracle, Q4_1, k, f_max, 1)
    u = lvk.layer_swiglu(Q4_1, 1, c["w1"][:f], c["w3"][:f], k, c["g"], c["x"], want="u")
    assert_rows_equal(u, c["u"][:, :f], "launch_matvec_cu EPI_SWIGLU_F32 q4_1 k=%d f=%d" % (k, f))


RESID = [(inp, k, m, e + 8) for inp, k, e in [(1, 6656, 6656), (1, 8192, 8192), (0, 17920, 6656), (0, 22016, 8192)]
         for m in (72, e, e + 8)]


@pytest.mark.parametrize("inp,k,m,m_max", RESID, ids=["in%d-k%d-m%d" % t[:3] for t in RESID])
def test_resid(lvk, oracle, inp, k, m, m_max):
    """EPI_RESID: PRO_ACTQ (Wo, input 1) and PRO_ACTF (W2, input 0)"""
    c = R.resid_case(oracle, Q4_1, k, m_max, 1)
    y = lvk.layer_resid(Q4_1, 1, c["w"][:m], k, c["a"], c["y0"][:, :m], input=inp)
    assert_rows_equal(y, c["ref"][:, :m], "launch_matvec_cu EPI_RESID q4_1 input=%d k=%d m=%d" % (inp, k, m))


@pytest.mark.parametrize("m,k", [(72, 6656), (32000, 6656), (72, 8192), (72, 17920), (72, 22016)])
def test_mul_mat_pairs(lvk, oracle, m, k):
    """lm_head (PRO_NORM + EPI_STORE) and the plain operator (PRO_ACTF + EPI_STORE), n = 1, through
    launch_matvec_auto"""
    rng = np.random.default_rng(m + 3 * k)
    w = R.make_weights(rng, Q4_1, m, k)
    x = (rng.standard_normal((1, k)) * 2.0).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    want = R.dots(oracle, Q4_1, w, R.convert(oracle, Q4_1, R.norm_rows(oracle, x, g)), k)
    assert_rows_equal(lvk.mul_mat_q_norm(Q4_1, w, m, k, g, x), want, "mul_mat_q_norm m=%d k=%d" % (m, k))
    want = R.dots(oracle, Q4_1, w, R.convert(oracle, Q4_1, x), k)
    assert_rows_equal(lvk.mul_mat_q(Q4_1, w, m, k, x), want, "mul_mat_q m=%d k=%d" % (m, k))


def test_refuses_a_pair_it_has_not(lvk, oracle):
    """PRO_NORM + EPI_QKV at k = 17920 has no instantiation: refused on the host ahead of any launch.  The
    entry point is called on the test's own buffers: it fails, the q16 row and both caches keep their
    bits, and a good call afterwards still matches"""
    E, H, k = 256, 2, 17920
    bad = R.qkv_case(oracle, Q4_1, k, E, H, 1)
    p = lambda a: a.ctypes.data
    w = np.ascontiguousarray(bad["w"])
    kc, vc, q16 = bad["kc0"].copy(), bad["vc0"].copy(), np.full(E, 0xA5A5, np.uint16)
    rc = lvk.lib.lvk_layer_qkv(Q4_1, 1, p(w), E, H, k, p(bad["g"]), p(bad["x"]), 1, R.N_CTX, 7, 1, p(kc), p(vc), p(q16))
    assert rc != 0
    assert np.array_equal(kc, bad["kc0"]) and np.array_equal(vc, bad["vc0"]) and (q16 == 0xA5A5).all()
    c = R.resid_case(oracle, Q4_1, k, 72, 1)
    y = lvk.layer_resid(Q4_1, 1, c["w"], k, c["a"], c["y0"], input=0)
    assert np.array_equal(bits(y), bits(c["ref"]))
