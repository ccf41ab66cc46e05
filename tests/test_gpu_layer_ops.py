"""Operator-level parity of the fused steps of a layer (lvk_layer_qkv / _resid / _swiglu / _ffn,
lvk_embed_rows: the (prologue, epilogue) pairs lvk_context.cpp enqueue_forward launches) against
the CPU oracle.  Every comparison is bit equality: uint32 views of f32, raw uint16 of q16 and of
the whole caches, raw block bytes.  Inputs, expected values and the shapes are tests/layer_ref.py's
(checked on the CPU by tests/test_layer_ref.py); a failure names the launcher path, the shape and
the first differing row.

path 1  launch_matvec_cu: the CU-balanced decode kernels (matvec_cu.hip, matvec_cu41.hip) and the one
        f16 / f32 matvec.  M per kernel from its row-group split: 72 rows (9 groups, fewer than
        workgroups), the model's M, and one group more (on 256 compute units K = 11008 Q4_0 then
        takes the 8-wave fallback instantiation, K = 4096 EPI_RESID the cross-group prefetch)
path 2  launch_matvec: the generic kernels, 1..15 tokens (partial 4- and 2-token groups)
path 3  launch_act + launch_mm: 16-token MFMA tiles, partial at 17, 33 and 40 tokens

What enqueue_forward launches, and the test that reaches it:
  QKV    single token  PRO_NORM + EPI_QKV                    test_decode_qkv, test_generic_qkv
         batch         EPI_ROPE_KV; EPI_STORE + launch_rope_kv  test_batched_qkv (fused 1 / 0)
  Wo     single token  PRO_ACTQ (Q4) / PRO_ACTF + EPI_RESID  test_decode_resid (in1; f16, f32), test_generic_resid
         batch         launch_actq_to_image / launch_act + EPI_RESID  test_batched_resid (in1 / in0)
  W1|W3  single token  PRO_NORM + EPI_SWIGLU_F32 / EPI_SWIGLU  test_decode_swiglu / test_generic_swiglu_blocks
         batch         EPI_SWIGLU_F32 / EPI_SWIGLU_Q          test_batched_swiglu, test_batched_ffn_pair
  W2     single token  PRO_ACTF (K = n_ff) / PRO_ACTQ + EPI_RESID  test_decode_resid (in0), test_generic_resid
         batch         EPI_RESID                              test_batched_resid, test_batched_ffn_pair
  embed                launch_embed                           test_embed_rows
Which instantiation a path-1 case takes depends on the device's compute units.  On 256: Q4_0 K = 11008
m = 4104 takes go<8, 0, 4, PRO_ACTF, EPI_RESID, 11008> (three row groups in a workgroup, the two-wave
kernel refuses), m = 72 and 4096 the two-wave kernel with its prologue waves; the row groups of a wave
run behind the cross-group prefetch for EPI_RESID at K = 4096 m = 4104, K = 8192 m = 8200 and
K = 22016 m = 8200, EPI_QKV at K = 4096 n_embd = 8192, EPI_SWIGLU_F32 at K = 4096 f = 13824 (Q4_0) and
f = 11008 (Q4_1), K = 5120 f = 13824.  The Q4_0 K = 8192 QKV / W1|W3 kernels run one row group per wave in
every case here.
"""
import numpy as np
import pytest

import layer_ref as R
from layer_ref import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def tname(t):
    return R.TYPE_NAME[t]


def first_diff(got, want):
    """(row, column) of the first differing element of two [n][m] arrays, as text"""
    d = np.argwhere(np.asarray(got) != np.asarray(want))
    return "none" if len(d) == 0 else "first difference at row %d, column %d of %d differing" % (d[0][0], d[0][-1], len(d))


def assert_rows_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype == np.float32:
        got, want = bits(got), bits(want)
    assert np.array_equal(got, want), "%s: %s" % (what, first_diff(got, want))


def check_qkv(lvk, oracle, c, path, n, fused, what):
    for n_past in R.n_past_set(n):
        want_q, want_k, want_v = R.qkv_expected(oracle, c, n, n_past)
        q16, kc, vc = lvk.layer_qkv(c["wtype"], path, c["w"], c["E"], c["H"], c["k"], c["g"], c["x"][:n], R.N_CTX, n_past,
                                    c["kc0"], c["vc0"], fused=fused)
        w = "%s n=%d n_past=%d fused=%d" % (what, n, n_past, fused)
        assert_rows_equal(q16, want_q, w + " q16")
        E = c["E"]
        assert_rows_equal(kc.reshape(R.N_CTX, E)[n_past:n_past + n], want_k.reshape(R.N_CTX, E)[n_past:n_past + n], w + " K rows")
        assert_rows_equal(vc.reshape(E, R.N_CTX)[:, n_past:n_past + n].T, want_v.reshape(E, R.N_CTX)[:, n_past:n_past + n].T,
                          w + " V columns")
        # the whole caches: the written cells and every bit beside them
        assert np.array_equal(kc, want_k), w + " K cache beside the written rows"
        assert np.array_equal(vc, want_v), w + " V cache beside the written columns"


# ---- decode, n = 1, path 1

@pytest.mark.parametrize("wtype,k,E,H", R.DECODE_QKV, ids=["%s-k%d-e%d" % (tname(t), k, e) for t, k, e, _ in R.DECODE_QKV])
def test_decode_qkv(lvk, oracle, wtype, k, E, H):
    """PRO_NORM + EPI_QKV of the decode kernels: RoPE at positions 0, 7 and n_ctx - 1 = 159, the q16
    row, the K row, the V column at a context that is no power of two, an all-zero K pair"""
    c = R.qkv_case(oracle, wtype, k, E, H, 1)
    check_qkv(lvk, oracle, c, 1, 1, 1, "launch_matvec_cu EPI_QKV %s k=%d n_embd=%d" % (tname(wtype), k, E))
    if not R.is_q4(wtype):
        # path 0 is the same kernel for a single token
        check_qkv(lvk, oracle, c, 0, 1, 1, "launch_matvec_auto EPI_QKV %s k=%d" % (tname(wtype), k))


SWIGLU_CASES = [(t, k, f, max(fs)) for t, k, fs in R.DECODE_SWIGLU for f in fs]


@pytest.mark.parametrize("wtype,k,f,f_max", SWIGLU_CASES, ids=["%s-k%d-f%d" % (tname(t), k, f) for t, k, f, _ in SWIGLU_CASES])
def test_decode_swiglu(lvk, oracle, wtype, k, f, f_max):
    """PRO_NORM + EPI_SWIGLU_F32 on the interleave-by-4 W1|W3 image: u in f32, with +-0 products, a zero
    block and a1 over the whole silu table"""
    c = R.swiglu_case(oracle, wtype, k, f_max, 1)
    u = lvk.layer_swiglu(wtype, 1, c["w1"][:f], c["w3"][:f], k, c["g"], c["x"], want="u")
    assert_rows_equal(u, c["u"][:, :f], "launch_matvec_cu EPI_SWIGLU_F32 %s k=%d f=%d (rows = W1|W3 outputs)" % (tname(wtype), k, f))


RESID_CASES = [(t, i, k, m, max(ms)) for t, i, k, ms in R.DECODE_RESID for m in ms]


@pytest.mark.parametrize("wtype,inp,k,m,m_max", RESID_CASES,
                         ids=["%s-in%d-k%d-m%d" % (tname(t), i, k, m) for t, i, k, m, _ in RESID_CASES])
def test_decode_resid(lvk, oracle, wtype, inp, k, m, m_max):
    """EPI_RESID of the decode kernels: PRO_ACTQ (the Wo role, input 1) and PRO_ACTF (the W2 role with
    its prologue waves; f16 / f32), y holding +-0, 1e30, 1e-30 and a zero weight row under y = -0.0"""
    c = R.resid_case(oracle, wtype, k, m_max, 1)
    y = lvk.layer_resid(wtype, 1, c["w"][:m], k, c["a"], c["y0"][:, :m], input=inp)
    pro = "PRO_ACTQ" if inp else "PRO_ACTF"
    assert_rows_equal(y, c["ref"][:, :m], "launch_matvec_cu %s EPI_RESID %s k=%d m=%d (columns = weight rows)" % (pro, tname(wtype), k, m))
    if inp == 1 or not R.is_q4(wtype):
        y = lvk.layer_resid(wtype, 0, c["w"][:m], k, c["a"], c["y0"][:, :m], input=inp)
        assert_rows_equal(y, c["ref"][:, :m], "launch_matvec_auto %s EPI_RESID %s k=%d m=%d" % (pro, tname(wtype), k, m))


@pytest.mark.parametrize("wtype", [R.F16, R.F32], ids=tname)
def test_decode_resid_refuses_partial_row_group(lvk, oracle, wtype):
    """the f16 / f32 EPI_RESID kernels take no M % 8 != 0 (only their EPI_STORE does): m = 250 is
    refused on the host, and a valid call afterwards still matches"""
    c = R.resid_case(oracle, wtype, 256, 72, 1)
    w250 = np.zeros((250, 256), c["w"].dtype)
    with pytest.raises(RuntimeError):
        lvk.layer_resid(wtype, 1, w250, 256, c["a"], np.zeros((1, 250), np.float32))
    y = lvk.layer_resid(wtype, 1, c["w"][:8], 256, c["a"], c["y0"][:, :8])
    assert_rows_equal(y, c["ref"][:, :8], "launch_matvec_cu PRO_ACTF EPI_RESID %s m=8" % tname(wtype))


# ---- the generic kernels, path 2

@pytest.mark.parametrize("k", R.GEN_K)
@pytest.mark.parametrize("wtype", [R.Q4_0, R.Q4_1], ids=tname)
def test_generic_qkv(lvk, oracle, wtype, k):
    """PRO_NORM + EPI_QKV of matvec_q4.hip / matvec_q41.hip for 1..15 tokens, fused and as EPI_STORE +
    launch_rope_kv"""
    c = R.qkv_case(oracle, wtype, k, R.GEN_E, R.GEN_H, max(R.N_GEN))
    for n in R.N_GEN:
        check_qkv(lvk, oracle, c, 2, n, 1, "launch_matvec EPI_QKV %s k=%d" % (tname(wtype), k))
    check_qkv(lvk, oracle, c, 2, 5, 0, "launch_matvec EPI_STORE + launch_rope_kv %s k=%d" % (tname(wtype), k))


@pytest.mark.parametrize("k", R.GEN_K)
@pytest.mark.parametrize("wtype", [R.Q4_0, R.Q4_1], ids=tname)
def test_generic_swiglu_blocks(lvk, oracle, wtype, k):
    """PRO_NORM + EPI_SWIGLU: the quantized u rows, block 1 of every row through the id = 0 branch"""
    c = R.swiglu_case(oracle, wtype, k, R.GEN_F, max(R.N_GEN))
    for n in R.N_GEN:
        blocks = lvk.layer_swiglu(wtype, 2, c["w1"], c["w3"], k, c["g"], c["x"][:n], want="blocks")
        assert_rows_equal(blocks, R.swiglu_blocks(oracle, c, n, R.GEN_F),
                          "launch_matvec EPI_SWIGLU %s k=%d n=%d (block bytes)" % (tname(wtype), k, n))


@pytest.mark.parametrize("k,ns", [(k, R.N_GEN) for k in R.GEN_K] + [(R.GEN_RESID_LONG[0], [R.GEN_RESID_LONG[1]])],
                         ids=["k%d" % k for k in R.GEN_K + [R.GEN_RESID_LONG[0]]])
@pytest.mark.parametrize("wtype", [R.Q4_0, R.Q4_1], ids=tname)
def test_generic_resid(lvk, oracle, wtype, k, ns):
    """PRO_ACTQ + EPI_RESID of the generic kernels (the Wo role, and W2 of a short batch)"""
    c = R.resid_case(oracle, wtype, k, R.GEN_M, max(R.N_GEN))
    for n in ns:
        y = lvk.layer_resid(wtype, 2, c["w"], k, c["a"][:n], c["y0"][:n], input=1)
        assert_rows_equal(y, c["ref"][:n], "launch_matvec PRO_ACTQ EPI_RESID %s k=%d n=%d" % (tname(wtype), k, n))
        if n > 1:
            y = lvk.layer_resid(wtype, 0, c["w"], k, c["a"][:n], c["y0"][:n], input=1)
            assert_rows_equal(y, c["ref"][:n], "path 0 PRO_ACTQ EPI_RESID %s k=%d n=%d" % (tname(wtype), k, n))


# ---- the batched route, path 3

def batch_ns(wtype):
    return R.N_BATCH if R.is_q4(wtype) else R.N_BATCH_F


BATCH_QKV = [(t, k, fused, a16) for t in R.ALL_TYPES for k in R.BATCH_K
             for fused in ((1, 0) if R.is_q4(t) else (0,)) for a16 in (("1", "0") if t == R.Q4_0 else (None,))]


@pytest.mark.parametrize("wtype,k,fused,a16", BATCH_QKV,
                         ids=["%s-k%d-fused%d%s" % (tname(t), k, fu, "" if a is None else "-a16_" + a) for t, k, fu, a in BATCH_QKV])
def test_batched_qkv(lvk, oracle, monkeypatch, wtype, k, fused, a16):
    """launch_act + launch_mm: EPI_ROPE_KV (Q4, fused) and EPI_STORE + launch_rope_kv, partial 16-token
    tiles, Q4_0 on the f16 A image and on the nibble image"""
    if a16 is not None:
        monkeypatch.setenv("LVK_PROMPT_A16", a16)
    c = R.qkv_case(oracle, wtype, k, R.BATCH_E, R.BATCH_H, R.N_MAX)
    epi = "EPI_ROPE_KV" if fused else "EPI_STORE + launch_rope_kv"
    for n in batch_ns(wtype):
        check_qkv(lvk, oracle, c, 3, n, fused, "launch_mm %s %s k=%d" % (epi, tname(wtype), k))
    check_qkv(lvk, oracle, c, 0, 17, fused, "path 0 %s %s k=%d" % (epi, tname(wtype), k))


BATCH_RESID = [(t, k, i) for t in R.ALL_TYPES for k in R.BATCH_K for i in ((1, 0) if R.is_q4(t) else (0,))]


@pytest.mark.parametrize("wtype,k,inp", BATCH_RESID, ids=["%s-k%d-in%d" % (tname(t), k, i) for t, k, i in BATCH_RESID])
def test_batched_resid(lvk, oracle, wtype, k, inp):
    """EPI_RESID of the batched matmuls after launch_act (input 0) or launch_actq_to_image (input 1):
    every row, the last token of a partial tile included"""
    c = R.resid_case(oracle, wtype, k, R.BATCH_M, R.N_MAX)
    for n in batch_ns(wtype):
        y = lvk.layer_resid(wtype, 3, c["w"], k, c["a"][:n], c["y0"][:n], input=inp)
        assert_rows_equal(y, c["ref"][:n], "launch_mm EPI_RESID %s k=%d n=%d input=%d" % (tname(wtype), k, n, inp))


@pytest.mark.parametrize("k", R.BATCH_K)
@pytest.mark.parametrize("wtype", R.ALL_TYPES, ids=tname)
def test_batched_swiglu(lvk, oracle, wtype, k):
    """EPI_SWIGLU_F32 of the batched matmuls"""
    c = R.swiglu_case(oracle, wtype, k, R.BATCH_F, R.N_MAX)
    for n in batch_ns(wtype):
        u = lvk.layer_swiglu(wtype, 3, c["w1"], c["w3"], k, c["g"], c["x"][:n], want="u")
        assert_rows_equal(u, c["u"][:n], "launch_mm EPI_SWIGLU_F32 %s k=%d n=%d" % (tname(wtype), k, n))


FFN_CASES = [(t, q) for t in R.ALL_TYPES for q in ((0, 1) if t == R.Q4_0 else (0,))]


@pytest.mark.parametrize("wtype,swiglu_q", FFN_CASES, ids=["%s-swiglu_q%d" % (tname(t), q) for t, q in FFN_CASES])
def test_batched_ffn_pair(lvk, oracle, wtype, swiglu_q):
    """the batch FFN pair as a context runs it: EPI_SWIGLU_Q into W2's operand image (Q4_0), or
    EPI_SWIGLU_F32 + launch_act, then EPI_RESID; every row of x is compared"""
    c = R.ffn_case(oracle, wtype, R.FFN_K, R.FFN_F, R.N_MAX)
    for n in batch_ns(wtype):
        x = lvk.layer_ffn(wtype, c["w1"], c["w3"], c["w2"], R.FFN_K, c["g"], c["x"][:n], swiglu_q=swiglu_q)
        assert_rows_equal(x, c["ref"][:n], "FFN pair %s swiglu_q=%d n=%d" % (tname(wtype), swiglu_q, n))


# ---- embed

@pytest.mark.parametrize("n_embd", R.EMBED_E)
@pytest.mark.parametrize("wtype", R.ALL_TYPES, ids=tname)
def test_embed_rows(lvk, oracle, wtype, n_embd):
    """launch_embed: the first and the last row of the table, a repeated token, Q4 rows with a d = 0 block"""
    c = R.embed_case(oracle, wtype, n_embd)
    x = lvk.embed_rows(wtype, c["emb"], n_embd, c["tokens"])
    assert_rows_equal(x, c["ref"], "launch_embed %s n_embd=%d (rows = tokens)" % (tname(wtype), n_embd))


# ---- refusals: one test per entry point; nothing is launched, a valid call afterwards still matches

def refused(fn, *args, **kw):
    with pytest.raises(RuntimeError):
        fn(*args, **kw)


def test_layer_qkv_bad_arguments(lvk, oracle):
    c = R.qkv_case(oracle, R.Q4_0, 256, R.GEN_E, R.GEN_H, max(R.N_GEN))
    E, H, C = R.GEN_E, R.GEN_H, R.N_CTX

    def call(wtype=R.Q4_0, path=2, w=c["w"], E_=E, H_=H, k=256, g=c["g"], x=c["x"][:2], n_ctx=C, n_past=3, kc=c["kc0"],
             vc=c["vc0"], fused=1, n=None):
        return lvk.layer_qkv(wtype, path, w, E_, H_, k, g, x, n_ctx, n_past, kc, vc, fused=fused, n=n)

    for wtype in (-1, 4, 7):
        refused(call, wtype=wtype)                                   # a bad type
    refused(call, path=4)
    refused(call, path=-1)
    refused(call, k=288, x=np.zeros((2, 288), np.float32), g=np.zeros(288, np.float32))      # k % 256 != 0
    refused(call, k=0, n=2)
    refused(call, n_past=C - 1)                                      # n_past + n > n_ctx
    refused(call, n_past=-1)
    refused(call, path=1)                                            # path 1 with n > 1
    refused(call, n=0)
    refused(call, fused=2)
    refused(call, H_=3)                                              # n_embd % n_head != 0
    refused(call, E_=40, H_=1)                                       # n_embd % 32 != 0
    refused(call, wtype=R.F16, path=3, fused=1)                      # f16 weights have no EPI_ROPE_KV
    for null in ("w", "g", "x", "kc", "vc"):                         # a null required pointer
        refused(call, n=2, **{null: None})
    q16, kc, vc = call()
    want_q, want_k, want_v = R.qkv_expected(oracle, c, 2, 3)
    assert np.array_equal(q16, want_q) and np.array_equal(kc, want_k) and np.array_equal(vc, want_v)


def test_layer_resid_bad_arguments(lvk, oracle):
    c = R.resid_case(oracle, R.Q4_0, 256, R.GEN_M, max(R.N_GEN))

    def call(wtype=R.Q4_0, path=2, w=c["w"], k=256, a=c["a"][:2], y=c["y0"][:2], inp=1, n=None, m=None):
        return lvk.layer_resid(wtype, path, w, k, a, y, input=inp, n=n, m=m)

    for wtype in (-1, 4):
        refused(call, wtype=wtype)
    refused(call, path=5)
    refused(call, k=288, a=np.zeros((2, 288), np.float32))
    refused(call, path=1)                                            # path 1 with n > 1
    refused(call, n=0)
    refused(call, inp=2)
    refused(call, wtype=R.F16, inp=1)                                # quantized input to f16 weights
    refused(call, m=60)                                              # m % 8 != 0
    refused(call, path=3)                                            # the Q4 batched matmul needs 128 | m
    for null in ("w", "a", "y"):
        refused(call, n=2, m=R.GEN_M, **{null: None})
    assert np.array_equal(bits(call()), bits(c["ref"][:2]))


def test_layer_swiglu_bad_arguments(lvk, oracle):
    c = R.swiglu_case(oracle, R.Q4_0, 256, R.GEN_F, max(R.N_GEN))

    def call(wtype=R.Q4_0, path=2, w1=c["w1"], w3=c["w3"], k=256, g=c["g"], x=c["x"][:2], want="blocks", n=None, f=None):
        return lvk.layer_swiglu(wtype, path, w1, w3, k, g, x, want=want, n=n, f=f)

    for wtype in (-1, 4):
        refused(call, wtype=wtype)
    refused(call, path=4)
    refused(call, k=288, x=np.zeros((2, 288), np.float32), g=np.zeros(288, np.float32))
    refused(call, path=1, want="u")                                  # path 1 with n > 1
    refused(call, n=0)
    refused(call, want="u")                                          # the output path 2 does not produce
    refused(call, want="both")
    refused(call, want="none")
    refused(call, path=3, want="blocks", x=c["x"][:5])               # ... nor path 3 blocks
    refused(call, path=1, want="blocks", x=c["x"][:1])
    refused(call, wtype=R.F16, path=2)                               # quantized output of f16 weights
    refused(call, f=62)
    for null in ("w1", "w3", "g", "x"):
        refused(call, n=2, f=R.GEN_F, **{null: None})
    assert np.array_equal(call(), R.swiglu_blocks(oracle, c, 2, R.GEN_F))


def test_layer_ffn_bad_arguments(lvk, oracle):
    c = R.ffn_case(oracle, R.Q4_0, R.FFN_K, R.FFN_F, R.N_MAX)
    c41 = R.ffn_case(oracle, R.Q4_1, R.FFN_K, R.FFN_F, R.N_MAX)

    def call(wtype=R.Q4_0, w1=c["w1"], w3=c["w3"], w2=c["w2"], k=R.FFN_K, g=c["g"], x=c["x"][:17], swiglu_q=1, n=None, f=None):
        return lvk.layer_ffn(wtype, w1, w3, w2, k, g, x, swiglu_q=swiglu_q, n=n, f=f)

    for wtype in (-1, 4):
        refused(call, wtype=wtype)
    refused(call, k=288, x=np.zeros((2, 288), np.float32))
    refused(call, f=760)                                             # f % 256 != 0
    refused(call, n=0)
    refused(call, swiglu_q=2)
    for wtype in (R.Q4_1, R.F16, R.F32):                             # swiglu_q = 1 on a type other than Q4_0
        refused(call, wtype=wtype, w1=c41["w1"], w3=c41["w3"], w2=c41["w2"])
    for null in ("w1", "w3", "w2", "g", "x"):
        refused(call, n=17, f=R.FFN_F, **{null: None})
    assert np.array_equal(bits(call()), bits(c["ref"][:17]))


def test_embed_rows_bad_arguments(lvk, oracle):
    c = R.embed_case(oracle, R.Q4_1, 128)

    def call(wtype=R.Q4_1, emb=c["emb"], n_embd=128, tokens=c["tokens"], n_vocab=None):
        return lvk.embed_rows(wtype, emb, n_embd, tokens, n_vocab=n_vocab)

    for wtype in (-1, 4):
        refused(call, wtype=wtype)
    refused(call, tokens=[0, R.EMBED_VOCAB])                         # a token id outside 0..n_vocab-1
    refused(call, tokens=[-1])
    refused(call, tokens=[])
    refused(call, n_embd=100)
    refused(call, n_vocab=0)
    refused(call, emb=None, n_vocab=R.EMBED_VOCAB)
    refused(call, tokens=None)
    assert np.array_equal(bits(call()), bits(c["ref"]))
