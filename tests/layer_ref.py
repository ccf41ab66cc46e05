"""Inputs and expected values of the layer operator tests (tests/test_gpu_layer_ops.py), built from
oracle pieces only; no GPU import.  tests/test_layer_ref.py checks on the CPU that every case holds
the edge it is there for.

The steps, each a function tests/test_oracle_golden.py pins or an existing restatement:
  norm      orc_rms_norm, then the f32 multiply by g
  convert   Q4: oracle.quantize; f16: orc_fp32_to_fp16; f32: the row itself
  dot       Q4: orc_vec_dot_q4_0 / _q4_1; f16: orc_vec_dot_f16; f32: f32_restatement.dot_f32
  RoPE      orc_rope at n_past + t; q16, the K row and the V column through orc_fp32_to_fp16
  residual  one f32 add of the dot and the old y
  SwiGLU    orc_silu(a1) * a3 in f32; blocks: oracle.quantize of the u row
  embed     oracle.dequantize of the row (Q4), the exact f16 widening, or the f32 row

A case is built once per process (memo) and shared; nothing modifies it.  Tests slice rows: the
first m weight rows and the first n input rows of a case give the first [n][m] results.
"""
import ctypes as C

import numpy as np

from f32_restatement import dot_f32

F32, F16, Q4_0, Q4_1 = 0, 1, 2, 3
BLOCK_BYTES = {Q4_0: 20, Q4_1: 24}
TYPE_NAME = {F32: "f32", F16: "f16", Q4_0: "q4_0", Q4_1: "q4_1"}
N_CTX = 160                    # a multiple of 32 that is no power of two

_memo = {}


def memo(fn):
    def wrapped(oracle, *key):
        k = (fn.__name__,) + key
        if k not in _memo:
            _memo[k] = fn(oracle, *key)
        return _memo[k]
    wrapped.__name__ = fn.__name__
    return wrapped


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f16_bits(oracle, x):
    """the oracle's GGML_FP32_TO_FP16 of every element"""
    conv = oracle.lib.orc_fp32_to_fp16
    return np.array([conv(float(v)) for v in np.asarray(x, np.float32).ravel()], np.uint16)


def is_q4(wtype):
    return wtype in (Q4_0, Q4_1)


# ---- weights

# rms of a weight: Q4 d ~ 0.02 |normal| times a centred nibble (rms ~4.6), f16 / f32 N(0, 0.02)
W_RMS = {F32: 0.02, F16: 0.02, Q4_0: 0.092, Q4_1: 0.092}


def make_weights(rng, wtype, m, k):
    """m rows of k weights in file layout.  Q4: random blocks directly (random nibble bytes, d drawn as
    0.02 |normal|; Q4_1 m near -7.5 d, so the values centre on zero): uint8 [m][k/32 * block bytes].
    f16: uint16 bits [m][k]; f32 [m][k]"""
    if wtype == F32:
        return (rng.standard_normal((m, k), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    if wtype == F16:
        return (rng.standard_normal((m, k), dtype=np.float32) * np.float32(0.02)).astype(np.float16).view(np.uint16)
    nb, bb = k // 32, BLOCK_BYTES[wtype]
    w = np.empty((m, nb, bb), np.uint8)
    d = (0.02 * np.abs(rng.standard_normal((m, nb), dtype=np.float32))).astype(np.float32)
    w[:, :, 0:4] = d.view(np.uint8).reshape(m, nb, 4)
    if wtype == Q4_1:
        mn = (-7.5 * d * (1 + 0.1 * rng.standard_normal((m, nb), dtype=np.float32))).astype(np.float32)
        w[:, :, 4:8] = mn.view(np.uint8).reshape(m, nb, 4)
    w[:, :, bb - 16:] = rng.integers(0, 256, (m, nb, 16), dtype=np.uint8)
    return w.reshape(m, nb * bb)


def zero_rows(wtype, w, rows):
    """make the given rows all-zero weights (Q4: d = 0 and m = 0 in every block, the nibbles stay)"""
    if not is_q4(wtype):
        w[rows] = 0
        return
    bb = BLOCK_BYTES[wtype]
    v = w.reshape(w.shape[0], -1, bb)
    v[rows, :, :bb - 16] = 0


def dequant_rows(oracle, wtype, w, k):
    """the f32 values of file-layout rows (embed's expected values)"""
    if wtype == F32:
        return np.array(w, np.float32)
    if wtype == F16:
        return w.view(np.float16).astype(np.float32)        # exact widening
    return np.stack([oracle.dequantize(r, wtype, k) for r in w])


# ---- the steps

def norm_rows(oracle, x, g):
    """g * rms_norm(x[t]) (ggml.c:6024-6080 + llama.cpp:984)"""
    x = np.ascontiguousarray(x, np.float32)
    n, k = x.shape
    y = np.zeros_like(x)
    oracle.lib.orc_rms_norm(x, k, n, y)
    return (y * np.asarray(g, np.float32)[None, :]).astype(np.float32)


def convert(oracle, wtype, a):
    """the operand a kernel of this weight type makes of f32 rows a [n][k]"""
    a = np.ascontiguousarray(a, np.float32)
    if wtype == F32:
        return a
    if wtype == F16:
        return f16_bits(oracle, a).reshape(a.shape)
    return np.stack([oracle.quantize(r, wtype) for r in a])


def _raw(fn, res, *args):
    """the function behind a typed ctypes entry, called with plain addresses (no per-call array checks)"""
    return C.cast(fn, C.CFUNCTYPE(res, *args))


def dots(oracle, wtype, w, act, k):
    """[n][m] f32: the reference dot of every weight row with every converted input row"""
    if wtype == F32:
        return dot_f32(w, act)
    w = np.ascontiguousarray(w)
    act = np.ascontiguousarray(act)
    m, n = w.shape[0], act.shape[0]
    name = "orc_vec_dot_f16" if wtype == F16 else "orc_vec_dot_q4_%d" % (wtype - 2)
    fn = _raw(getattr(oracle.lib, name), C.c_float, C.c_int, C.c_void_p, C.c_void_p)
    out = np.zeros((n, m), np.float32)
    wb, ws = w.ctypes.data, w.strides[0]
    for t in range(n):
        xa = act.ctypes.data + t * act.strides[0]
        out[t] = [fn(k, wb + r * ws, xa) for r in range(m)]
    return out


def silu_mul(oracle, a1, a3):
    """ggml_vec_silu_f32's f16 table (ggml.c:2495), then ggml_mul in f32"""
    a1 = np.ascontiguousarray(a1, np.float32)
    s = np.zeros_like(a1)
    oracle.lib.orc_silu(a1.reshape(-1), a1.size, s.reshape(-1))
    return (s * np.asarray(a3, np.float32)).astype(np.float32)


# ---- cases

def _seed(*key):
    s = 17
    for v in key:
        s = (s * 1000003 + int(v)) % (1 << 31)
    return s


@memo
def resid_case(oracle, wtype, k, m_max, n_max):
    """y += W . conv(a): w [m_max][k] with row 3 all zero, a [n_max][k], y0 [n_max][m_max] with
    0.0, -0.0, 1e30, 1e-30 in cells 0, 1, 2, 4 of every row and -0.0 in cell 3 (the zero weight row),
    ordinary values elsewhere; dot and ref = dot + y0 [n_max][m_max]"""
    rng = np.random.default_rng(_seed(1, wtype, k, m_max, n_max))
    w = make_weights(rng, wtype, m_max, k)
    zero_rows(wtype, w, [3])
    a = (rng.standard_normal((n_max, k)) * (1 + np.arange(n_max) % 3)[:, None]).astype(np.float32)
    y0 = (rng.standard_normal((n_max, m_max)) * 3).astype(np.float32)
    y0[:, 0], y0[:, 1], y0[:, 2], y0[:, 3], y0[:, 4] = 0.0, -0.0, 1e30, -0.0, 1e-30
    dot = dots(oracle, wtype, w, convert(oracle, wtype, a), k)
    ref = (dot + y0).astype(np.float32)
    return dict(wtype=wtype, k=k, w=w, a=a, y0=y0, dot=dot, ref=ref)


ZERO_W1_ROW, ZERO_W3_ROW, ZERO_BLOCK = 1, 2, slice(32, 64)


@memo
def swiglu_case(oracle, wtype, k, f_max, n_max):
    """u = silu(W1 . a) * (W3 . a), a = conv(g * rms_norm(x)): W1 row 1 and W3 row 2 all zero (products
    of +-0), W3 rows 32..63 all zero (a zero block of u), g scaled so that a1 has a standard deviation
    near 10 (the silu table's flush-to-zero end below -20.5 and its identity end)"""
    rng = np.random.default_rng(_seed(2, wtype, k, f_max, n_max))
    w1 = make_weights(rng, wtype, f_max, k)
    w3 = make_weights(rng, wtype, f_max, k)
    zero_rows(wtype, w1, [ZERO_W1_ROW])
    zero_rows(wtype, w3, [ZERO_W3_ROW])
    zero_rows(wtype, w3, ZERO_BLOCK)
    g = (10.0 / (W_RMS[wtype] * np.sqrt(k)) * (1 + 0.1 * rng.standard_normal(k))).astype(np.float32)
    x = (rng.standard_normal((n_max, k)) * (0.5 + np.arange(n_max) % 4)[:, None]).astype(np.float32)
    act = convert(oracle, wtype, norm_rows(oracle, x, g))
    a1 = dots(oracle, wtype, w1, act, k)
    a3 = dots(oracle, wtype, w3, act, k)
    u = silu_mul(oracle, a1, a3)
    return dict(wtype=wtype, k=k, w1=w1, w3=w3, g=g, x=x, a1=a1, a3=a3, u=u)


def swiglu_blocks(oracle, case, n, f):
    """the quantized rows of u[:n, :f]: uint8 [n][f/32 * block bytes]"""
    return np.stack([oracle.quantize(np.ascontiguousarray(case["u"][t, :f]), case["wtype"]) for t in range(n)])


ZERO_K_PAIR = (4, 5)           # elements of K whose weight rows are all zero


@memo
def qkv_case(oracle, wtype, k, n_embd, n_head, n_max):
    """q | k | v = W . conv(g * rms_norm(x)): w [3 * n_embd][k] with the K rows of elements 4 and 5 (a
    RoPE pair) all zero; qkv [n_max][3 * n_embd] are the dots before RoPE; kc0 / vc0: caches of n_ctx =
    160 positions prefilled with random bits"""
    E = n_embd
    rng = np.random.default_rng(_seed(3, wtype, k, n_embd, n_head, n_max))
    w = make_weights(rng, wtype, 3 * E, k)
    zero_rows(wtype, w, [E + ZERO_K_PAIR[0], E + ZERO_K_PAIR[1]])
    g = (1.5 / (W_RMS[wtype] * np.sqrt(k)) * (1 + 0.1 * rng.standard_normal(k))).astype(np.float32)
    x = (rng.standard_normal((n_max, k)) * (0.5 + np.arange(n_max) % 4)[:, None]).astype(np.float32)
    qkv = dots(oracle, wtype, w, convert(oracle, wtype, norm_rows(oracle, x, g)), k)
    kc0 = rng.integers(0, 65536, N_CTX * E, dtype=np.uint16)
    vc0 = rng.integers(0, 65536, N_CTX * E, dtype=np.uint16)
    return dict(wtype=wtype, k=k, E=E, H=n_head, w=w, g=g, x=x, qkv=qkv, kc0=kc0, vc0=vc0, exp={})


def qkv_expected(oracle, case, n, n_past):
    """(q16 [n][E], kc, vc) after rows 0..n-1 were RoPE'd and appended at n_past.. (memo per case)"""
    key = (n, n_past)
    if key not in case["exp"]:
        E, H = case["E"], case["H"]
        hd = E // H
        q16 = np.zeros((n, E), np.uint16)
        kc, vc = case["kc0"].copy(), case["vc0"].copy()
        for t in range(n):
            row = case["qkv"][t]
            yq, yk = np.zeros(E, np.float32), np.zeros(E, np.float32)
            oracle.lib.orc_rope(np.ascontiguousarray(row[:E]), hd, H, 1, n_past + t, yq)
            oracle.lib.orc_rope(np.ascontiguousarray(row[E:2 * E]), hd, H, 1, n_past + t, yk)
            q16[t] = f16_bits(oracle, yq)
            kc.reshape(N_CTX, E)[n_past + t] = f16_bits(oracle, yk)
            vc.reshape(E, N_CTX)[:, n_past + t] = f16_bits(oracle, row[2 * E:])
        case["exp"][key] = (q16, kc, vc)
    return case["exp"][key]


@memo
def ffn_case(oracle, wtype, k, f, n_max):
    """the FFN pair x += W2 . conv(silu(W1 . a) * (W3 . a)): the SwiGLU case's edges, then W2 [k][f];
    ref [n_max][k]"""
    rng = np.random.default_rng(_seed(4, wtype, k, f, n_max))
    s = swiglu_case(oracle, wtype, k, f, n_max)
    w2 = make_weights(rng, wtype, k, f)
    dot = dots(oracle, wtype, w2, convert(oracle, wtype, s["u"]), f)
    ref = (dot + s["x"]).astype(np.float32)
    return dict(wtype=wtype, k=k, f=f, w1=s["w1"], w3=s["w3"], w2=w2, g=s["g"], x=s["x"], u=s["u"], dot=dot, ref=ref)


EMBED_TOKENS = [0, 63, 5, 5, 17]
EMBED_VOCAB = 64


@memo
def embed_case(oracle, wtype, n_embd):
    """emb [64][n_embd] rows in file layout (Q4: block 1 of rows 5 and 63 has d = 0), the tokens first,
    last and a repeat, and the expected rows"""
    rng = np.random.default_rng(_seed(5, wtype, n_embd))
    emb = make_weights(rng, wtype, EMBED_VOCAB, n_embd)
    if is_q4(wtype):
        bb = BLOCK_BYTES[wtype]
        emb.reshape(EMBED_VOCAB, -1, bb)[[5, 63], 1, 0:4] = 0
    tokens = np.array(EMBED_TOKENS, np.int32)
    ref = dequant_rows(oracle, wtype, emb, n_embd)[tokens]
    return dict(wtype=wtype, emb=emb, tokens=tokens, ref=ref)


# ---- the shapes of the GPU tests (tests/test_gpu_layer_ops.py) and of the CPU self-checks

N_GEN = [1, 2, 4, 5, 15]               # the generic kernels: 4 tokens per workgroup
N_BATCH = [16, 17, 33, 40]             # the batched route: 16 tokens per MFMA tile
N_BATCH_F = [2] + N_BATCH              # f16 / f32 weights batch from 2 tokens on
N_MAX = 40


def n_past_set(n):
    return [0, 7, N_CTX - n]


# decode, path 1: (type, k, n_embd, n_head)
# (n_embd = 8192 at k = 4096: 12 row groups per workgroup on 256 compute units, more than the
# kernels' 8 waves, so the QKV epilogue runs behind the cross-group prefetch)
DECODE_QKV = [(Q4_0, 4096, 4096, 32), (Q4_0, 8192, 1024, 8), (Q4_0, 4096, 8192, 64),
              (Q4_1, 5120, 5120, 40), (Q4_1, 4096, 4096, 32), (Q4_1, 4096, 1024, 8), (Q4_1, 4096, 8192, 64),
              (F16, 256, 256, 2), (F16, 4096, 256, 2), (F32, 256, 256, 2), (F32, 4096, 256, 2)]
# (type, k, [f...]): 9 x 8 row groups, the model's f, one row group more (f = 13824 at k = 4096: more
# row groups per workgroup than the Q4_0 kernel's 12 waves)
DECODE_SWIGLU = [(Q4_0, 4096, [288, 11008, 11012, 13824]), (Q4_0, 8192, [288]),
                 (Q4_1, 5120, [288, 13824, 13828]), (Q4_1, 4096, [288, 11008]),
                 (F16, 256, [72]), (F16, 4096, [72]), (F32, 256, [72]), (F32, 4096, [72])]
# (type, input, k, [m...])
DECODE_RESID = [(Q4_0, 1, 4096, [72, 4096, 4104]), (Q4_0, 1, 8192, [72, 8192, 8200]),
                (Q4_0, 0, 11008, [72, 4096, 4104]), (Q4_0, 0, 22016, [72, 8192, 8200]),
                (Q4_1, 1, 5120, [72, 5120, 5128]), (Q4_1, 0, 13824, [72, 5120, 5128]),
                (Q4_1, 1, 4096, [72, 4096]), (Q4_1, 0, 11008, [72, 4096]),
                (F16, 0, 256, [8, 72]), (F16, 0, 4096, [8, 72]), (F32, 0, 256, [8, 72]), (F32, 0, 4096, [8, 72])]
# generic kernels, path 2
GEN_K = [256, 4096]
GEN_E, GEN_H, GEN_F, GEN_M = 256, 2, 64, 64
GEN_RESID_LONG = (11008, 5)            # a row length compiled into the multi-token kernels
# batched route, path 3
BATCH_K = [256, 4096]
BATCH_E, BATCH_H, BATCH_F, BATCH_M = 256, 2, 128, 128
FFN_K, FFN_F = 256, 768
EMBED_E = [128, 4096]
ALL_TYPES = [F32, F16, Q4_0, Q4_1]
