"""The Q4_1 batched matmul on the octet image (mm_mfma41_nib.hip: a Q4_1 matrix without its f16 +
side images), bit for bit against the oracle's ggml_vec_dot_q4_1: the matmul alone, its four
epilogues through the layer entry points at path 3, and a model loaded under LVK_PROMPT_A16=0.
Every test first asserts that this kernel is what runs."""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import bits
from test_gpu_layer_ops import assert_rows_equal, check_qkv

pytestmark = pytest.mark.gpu
Q41 = R.Q4_1


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.fixture
def no_images(lvk, monkeypatch):
    monkeypatch.setenv("LVK_PROMPT_A16", "0")
    assert lvk.prompt_weight_source(Q41) == 1
    return lvk


# one partial chunk of 8 blocks; a full chunk + a partial one, ragged second token tile; 13B rows, 5
# chunks, two row tiles; 13.5 chunks; three row tiles (mm_tile's leftover path)
@pytest.mark.parametrize("m,k,n,norm", [(128, 256, 2, False), (128, 1280, 17, True), (256, 5120, 40, True),
                                        (128, 13824, 16, False), (384, 1024, 33, True)])
def test_mul_mat_q4_1_octet_image_bit_exact(lvk, oracle, m, k, n, norm):
    rng = np.random.default_rng(7 * m + k + 13 * n)
    w = (rng.standard_normal((m, k)) * 0.02).astype(np.float32)
    w[1, 32:64] = 0.01                                # a constant weight block (d = 0, m = 0.01)
    w[2, :32] = 0.0                                   # an all-zero weight block
    w[3, 64:96] = 0.05                                # 31 values at the maximum, the last at the minimum:
    w[3, 95] = -0.05                                  # group sums 120, 120, 120, 105
    wq = np.stack([oracle.quantize(r, 3, reference=True) for r in w])
    blk = wq[3].reshape(-1, 24)[2, 8:]
    assert [int((blk[4 * g:4 * g + 4] & 15).sum() + (blk[4 * g:4 * g + 4] >> 4).sum()) for g in range(4)] == [120, 120, 120, 105]
    x = (rng.standard_normal((n, k)) * 1.7).astype(np.float32)
    x[0, :32] = 0.0                                   # an all-zero activation block
    x[-1, 64:96] = -0.5                               # a constant activation block
    g = (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float32) if norm else None
    got = lvk.mul_mat_q_mfma(3, wq, m, k, x, g=g, images=False)
    xin = R.norm_rows(oracle, x, g) if norm else x
    want = R.dots(oracle, Q41, wq, R.convert(oracle, Q41, xin), k)
    assert_rows_equal(got, want, "mul_mat_q_mfma images=False m=%d k=%d n=%d" % (m, k, n))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("k", R.BATCH_K)
def test_octet_image_qkv(no_images, oracle, k, fused):
    """EPI_ROPE_KV (fused) and EPI_STORE + launch_rope_kv"""
    c = R.qkv_case(oracle, Q41, k, R.BATCH_E, R.BATCH_H, R.N_MAX)
    for n in R.N_BATCH:
        check_qkv(no_images, oracle, c, 3, n, fused, "octet image QKV k=%d" % k)


@pytest.mark.parametrize("inp", [0, 1])
@pytest.mark.parametrize("k", R.BATCH_K)
def test_octet_image_resid(no_images, oracle, k, inp):
    """EPI_RESID after launch_act (input 0) and launch_actq_to_image (input 1)"""
    c = R.resid_case(oracle, Q41, k, R.BATCH_M, R.N_MAX)
    for n in R.N_BATCH:
        y = no_images.layer_resid(Q41, 3, c["w"], k, c["a"][:n], c["y0"][:n], input=inp)
        assert_rows_equal(y, c["ref"][:n], "octet image EPI_RESID k=%d n=%d input=%d" % (k, n, inp))


@pytest.mark.parametrize("k", R.BATCH_K)
def test_octet_image_swiglu(no_images, oracle, k):
    """EPI_SWIGLU_F32 on the interleaved W1|W3 image"""
    c = R.swiglu_case(oracle, Q41, k, R.BATCH_F, R.N_MAX)
    for n in R.N_BATCH:
        u = no_images.layer_swiglu(Q41, 3, c["w1"], c["w3"], k, c["g"], c["x"][:n], want="u")
        assert_rows_equal(u, c["u"][:n], "octet image EPI_SWIGLU_F32 k=%d n=%d" % (k, n))


@pytest.mark.parametrize("n", [17, 33])
def test_octet_image_model_prompt_and_decode(no_images, oracle, tiny_models, n):
    """every role of a layer and the lm_head (logits_all rows), then four decode steps on the K / V
    the fused epilogue stored"""
    path = tiny_models["tiny_q4_1"]
    m = no_images.Llama(path, n_ctx=256, logits_all=True)
    om = oracle.model(path, 256)
    try:
        assert m.prompt_image_bytes() == 0
        assert m.prompt_batched(17) == 1
        toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, n)], np.int32)
        a, b = m.eval(toks, 0), om.eval(toks, 0, logits_all=True)
        assert a.shape[0] == n
        assert np.array_equal(bits(a), bits(b)), "prompt logits"
        n_past, tok = n, int(np.argmax(b[-1]))
        for _ in range(4):
            a, b = m.eval([tok], n_past), om.eval([tok], n_past, logits_all=True)
            assert np.array_equal(bits(a), bits(b)), "n_past %d" % n_past
            n_past, tok = n_past + 1, int(np.argmax(b[-1]))
    finally:
        m.close()
        om.close()
