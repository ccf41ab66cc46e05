"""Operator-level parity of the batched-decode rows kernels (attention_rows.hip: k_rope_kv_rows,
k_attn_rows<Q4_0|Q4_1>) and of the fused Wo quantizers of the other attention kernels against the
CPU oracle.  Every comparison is bit equality (uint32 views of f32, raw bytes of blocks and f16).

The reference of an attention row (slot, pos) is the oracle's single-token attention at
n_past = pos on that slot's layer: orc_attention(kc[slot][layer], vc[slot][layer], q, E, H, C, pos, 1),
and of its Wo blocks oracle.quantize of that row.

k_attn_rows switches code paths on n_kv = pos + 1:
  32 / 64   SIMD part n_kv & ~31 of the P.V dot empty / one step; K passes of 64 positions
  256       the softmax loops stride by 256 threads
  512       K is loaded in blocks of 512 positions (load_k(pb) with pb > 0 above)
  544       V steps 0..15 come from LDS, steps 16.. from global memory (n_kv >= 544); the double
            tail reads LDS for n_kv & ~31 < 512 and global memory at vc + vrow + (n_kv & ~31) above
  1024      a third K block
  n_ctx     the last row of the cache
"""
import itertools

import numpy as np
import pytest

from layer_ref import f16_bits

pytestmark = pytest.mark.gpu

E0, H0 = 512, 4
NAN16 = 0x7E00


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def make_caches(rng, n_slots, n_layer, C, E):
    """[n_slots][n_layer][C * E] f16 bits of standard normal values, K and V"""
    shape = (n_slots, n_layer, C * E)
    kc = rng.standard_normal(shape, dtype=np.float32).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal(shape, dtype=np.float32).astype(np.float16).view(np.uint16)
    return kc, vc


def oracle_rows(oracle, kc, vc, layer, q, slots, pos, E, H, C):
    """the reference rows [n][E] of (slots[i], pos[i])"""
    q = np.ascontiguousarray(q, np.float32).reshape(len(slots), E)
    want = np.zeros((len(slots), E), np.float32)
    for i, (s, p) in enumerate(zip(slots, pos)):
        oracle.lib.orc_attention(kc[s][layer], vc[s][layer], q[i], E, H, C, int(p), 1, want[i])
    return want


def check_rows(oracle, got, blocks, want, qt, pos):
    assert got.shape == want.shape and blocks.shape[0] == want.shape[0]
    for i in range(len(want)):
        assert np.array_equal(bits(got[i]), bits(want[i])), "row %d (pos %d)" % (i, pos[i])
        assert np.array_equal(blocks[i], oracle.quantize(want[i], qt)), "blocks of row %d (pos %d)" % (i, pos[i])


# ---- (a) one launch, every boundary

POS_A = [0, 30, 31, 32, 62, 63, 64, 254, 255, 256, 510, 511, 512, 542, 543, 544, 574, 1022, 1023, 1024, 1311,
         2046, 2047]


@pytest.fixture(scope="module")
def boundary_case(oracle):
    """caches, rows in a shuffled fixed order over 3 slots, and per q scale the queries and
    reference rows (computed once, shared by the type / exp-path cases, never modified)"""
    C, n_layer, layer, n_slots = 2048, 2, 1, 3
    rng = np.random.default_rng(2048)
    kc, vc = make_caches(rng, n_slots, n_layer, C, E0)
    order = np.random.RandomState(7).permutation(len(POS_A))
    pos = [POS_A[j] for j in order]
    slots = [int(j) % n_slots for j in range(len(pos))]
    assert sorted(pos) == POS_A and set(slots) == {0, 1, 2} and pos != POS_A
    base = rng.standard_normal((len(pos), E0))
    per_qs = {}
    for qs in (1, 8):
        q = (qs * base).astype(np.float32)
        per_qs[qs] = (q, oracle_rows(oracle, kc, vc, layer, q, slots, pos, E0, H0, C))
    return dict(C=C, layer=layer, kc=kc, vc=vc, slots=slots, pos=pos, per_qs=per_qs)


@pytest.mark.parametrize("exp_path", ["computed", "table"])
@pytest.mark.parametrize("qs", [1, 8])
@pytest.mark.parametrize("qt", [2, 3])
def test_rows_every_boundary_in_one_launch(lvk, oracle, boundary_case, monkeypatch, qt, qs, exp_path):
    """n_kv on and one position to each side of 32, 64, 256, 512, 544, 1024 and n_ctx = 2048 in one
    launch: later K blocks, V steps from global memory, the double tail from LDS and from global
    memory, the 256-thread softmax stride, layer_off != 0 and three slots; rows and Wo blocks of both
    block types, both exp paths; qs = 8 drives the softmax to exp arguments that underflow in f16"""
    if exp_path == "table":
        monkeypatch.setenv("LVK_EXP_TABLE", "1")
    c = boundary_case
    for b in (32, 64, 256, 512, 544, 1024):
        assert {b - 2, b - 1, b} <= set(c["pos"])          # n_kv = b - 1, b, b + 1
    assert {c["C"] - 2, c["C"] - 1} <= set(c["pos"])
    q, want = c["per_qs"][qs]
    got, blocks = lvk.attention_rows(qt, c["kc"], c["vc"], c["layer"], q, c["slots"], c["pos"], E0, H0, c["C"])
    check_rows(oracle, got, blocks, want, qt, c["pos"])


# ---- (b) nothing past pos reaches the result

POS_B = [0, 31, 100, 511, 512, 530, 543, 1000]


@pytest.fixture(scope="module")
def poison_case(oracle):
    """one slot per row; the reference is computed on the clean caches, the kernel gets copies
    whose K rows and V columns past the row's pos hold the f16 NaN 0x7e00"""
    C = 1024
    rng = np.random.default_rng(77)
    kc, vc = make_caches(rng, len(POS_B), 1, C, E0)
    slots = list(range(len(POS_B)))
    base = rng.standard_normal((len(POS_B), E0))
    per_qs = {}
    for qs in (1, 8):
        q = (qs * base).astype(np.float32)
        per_qs[qs] = (q, oracle_rows(oracle, kc, vc, 0, q, slots, POS_B, E0, H0, C))
    kp, vp = kc.copy(), vc.copy()
    for s, p in enumerate(POS_B):
        kp[s, 0].reshape(C, E0)[p + 1:] = NAN16
        vp[s, 0].reshape(E0, C)[:, p + 1:] = NAN16
    assert int(np.count_nonzero(kp[0] == NAN16)) >= (C - 1) * E0
    return dict(C=C, kc=kp, vc=vp, slots=slots, per_qs=per_qs)


@pytest.mark.parametrize("qs", [1, 8])
@pytest.mark.parametrize("qt", [2, 3])
def test_rows_read_nothing_past_pos(lvk, oracle, poison_case, qt, qs):
    """the state a rewound sequence leaves: positions > pos of the row's slot hold NaN.  The K
    loads clamp to n_kv - 1, P is zero-padded to a multiple of 32 and the double tail stops at
    n_kv, so no NaN may reach a row (the oracle gives the same finite rows with and without the
    poison; the reference here is the one without)"""
    c = poison_case
    q, want = c["per_qs"][qs]
    assert np.all(np.isfinite(want))
    got, blocks = lvk.attention_rows(qt, c["kc"], c["vc"], 0, q, c["slots"], POS_B, E0, H0, c["C"])
    assert np.all(np.isfinite(got))
    check_rows(oracle, got, blocks, want, qt, POS_B)


# ---- (c) per-row slot and position

def test_rows_index_their_own_slot_and_position(lvk, oracle):
    """two slots with different caches, one query for all four rows (slot 0, p), (slot 1, p),
    (slot 1, p'), (slot 0, p'): the references differ only through slot and position, pairwise,
    so a row that reads another row's slot or position cannot pass"""
    C, p, p2 = 1024, 40, 600
    rng = np.random.default_rng(5)
    kc, vc = make_caches(rng, 2, 1, C, E0)
    slots, pos = [0, 1, 1, 0], [p, p, p2, p2]
    q = np.tile(rng.standard_normal(E0).astype(np.float32), (4, 1))
    want = oracle_rows(oracle, kc, vc, 0, q, slots, pos, E0, H0, C)
    for i, j in itertools.combinations(range(4), 2):
        assert not np.array_equal(bits(want[i]), bits(want[j])), (i, j)
    for qt in (2, 3):
        got, blocks = lvk.attention_rows(qt, kc, vc, 0, q, slots, pos, E0, H0, C)
        check_rows(oracle, got, blocks, want, qt, pos)


# ---- (d) narrow contexts

@pytest.mark.parametrize("C,pos", [(128, [0, 95, 127]), (160, [127, 128, 159]), (544, [512, 542, 543])])
@pytest.mark.parametrize("qt", [2, 3])
def test_rows_narrow_contexts(lvk, oracle, qt, C, pos):
    """C = 128: the smallest context the kernel admits; C = 160: a multiple of 32 that is no
    multiple of 64, the V DMA of the last step and the LDS tail of pos 128 end at the row's end;
    C = 544: the double tail read from global memory (n_kv 513, 543) ends at the row's end.  The
    rows alternate over two slots of the second of two layers, so the last V row of slot 1 ends
    the allocation."""
    rng = np.random.default_rng(C)
    kc, vc = make_caches(rng, 2, 2, C, E0)
    slots = [1, 0, 1]
    q = (2 * rng.standard_normal((len(pos), E0))).astype(np.float32)
    want = oracle_rows(oracle, kc, vc, 1, q, slots, pos, E0, H0, C)
    got, blocks = lvk.attention_rows(qt, kc, vc, 1, q, slots, pos, E0, H0, C)
    check_rows(oracle, got, blocks, want, qt, pos)


# ---- (e) 65B head shape

def test_rows_65b_heads(lvk, oracle):
    """LLaMA-65B attention shape, 64 heads x 128: grid (64, 4, 2)"""
    E, H, C = 8192, 64, 512
    rng = np.random.default_rng(65)
    kc, vc = make_caches(rng, 2, 1, C, E)
    slots, pos = [0, 1, 1, 0], [0, 37, 300, 511]
    q = (2 * rng.standard_normal((4, E))).astype(np.float32)
    want = oracle_rows(oracle, kc, vc, 0, q, slots, pos, E, H, C)
    got, blocks = lvk.attention_rows(2, kc, vc, 0, q, slots, pos, E, H, C)
    check_rows(oracle, got, blocks, want, 2, pos)


# ---- (f) RoPE + KV append

ROWS_F = [(0, 0), (2, 255), (1, 17), (1, 18), (0, 128)]


@pytest.mark.parametrize("E,H,n_layer", [(512, 4, 2), (128, 1, 2), (384, 3, 2), (8192, 64, 1)])
def test_rope_kv_rows(lvk, oracle, E, H, n_layer):
    """k_rope_kv_rows: q16, the K rows and V columns it writes, and every other bit of both caches
    (the other layer, untouched positions, untouched slots) against orc_rope + the oracle's f16
    conversion.  E + E/2 pairs per row: 192 (less than one 256-thread block), 576 (a partial last
    block, the K / V boundary inside a block), 768 and 12288 (the 65B shape)."""
    C, n_slots, layer = 256, 3, n_layer - 1
    rng = np.random.default_rng(E + H)
    kc0 = rng.integers(0, 65536, (n_slots, n_layer, C * E), dtype=np.uint16)
    vc0 = rng.integers(0, 65536, (n_slots, n_layer, C * E), dtype=np.uint16)
    slots, pos = [s for s, _ in ROWS_F], [p for _, p in ROWS_F]
    n = len(ROWS_F)
    qkv = (1.5 * rng.standard_normal((n, 3 * E))).astype(np.float32)
    want_q = np.zeros((n, E), np.uint16)
    want_k, want_v = kc0.copy(), vc0.copy()
    for i, (s, p) in enumerate(ROWS_F):
        yq, yk = np.zeros(E, np.float32), np.zeros(E, np.float32)
        oracle.lib.orc_rope(np.ascontiguousarray(qkv[i, :E]), 128, H, 1, p, yq)
        oracle.lib.orc_rope(np.ascontiguousarray(qkv[i, E:2 * E]), 128, H, 1, p, yk)
        want_q[i] = f16_bits(oracle, yq)
        want_k[s, layer].reshape(C, E)[p] = f16_bits(oracle, yk)
        want_v[s, layer].reshape(E, C)[:, p] = f16_bits(oracle, qkv[i, 2 * E:])
    assert not np.array_equal(want_k, kc0) and not np.array_equal(want_v, vc0)
    keep_k, keep_v = kc0.copy(), vc0.copy()
    q16, got_k, got_v = lvk.rope_kv_rows(qkv, slots, pos, E, H, C, layer, kc0, vc0)
    assert np.array_equal(kc0, keep_k) and np.array_equal(vc0, keep_v)      # the wrapper works on copies
    assert np.array_equal(q16, want_q)
    for i, (s, p) in enumerate(ROWS_F):
        assert np.array_equal(got_k[s, layer].reshape(C, E)[p], want_k[s, layer].reshape(C, E)[p]), "K of row %d" % i
        assert np.array_equal(got_v[s, layer].reshape(E, C)[:, p], want_v[s, layer].reshape(E, C)[:, p]), "V of row %d" % i
    # the whole caches: the written cells and every bit beside them
    assert np.array_equal(got_k, want_k)
    assert np.array_equal(got_v, want_v)


# ---- (g) bad arguments

def test_rows_bad_arguments(lvk, oracle):
    """every bad argument is refused on the host (RuntimeError from rc -1) before anything is
    uploaded, for both entry points, and a valid call afterwards still matches"""
    C, n_slots, n_layer = 128, 2, 2
    rng = np.random.default_rng(9)
    kc, vc = make_caches(rng, n_slots, n_layer, C, E0)
    q2 = rng.standard_normal((2, E0)).astype(np.float32)
    qkv2 = rng.standard_normal((2, 3 * E0)).astype(np.float32)

    def attn(qt=2, slots=(0, 1), pos=(5, 100), layer=1, E=E0, H=H0, C_=C, kc_=kc, vc_=vc, q=q2):
        return lvk.attention_rows(qt, kc_, vc_, layer, q, list(slots), list(pos), E, H, C_)

    def rope(slots=(0, 1), pos=(5, 100), layer=1, E=E0, H=H0, C_=C, kc_=kc, vc_=vc, x=qkv2):
        return lvk.rope_kv_rows(x, list(slots), list(pos), E, H, C_, layer, kc_, vc_)

    empty_q, empty_x = np.zeros((0, E0), np.float32), np.zeros((0, 3 * E0), np.float32)
    kc96, vc96 = kc.reshape(-1)[:n_slots * n_layer * 96 * E0].reshape(n_slots, n_layer, -1), \
        vc.reshape(-1)[:n_slots * n_layer * 96 * E0].reshape(n_slots, n_layer, -1)
    bad = [
        dict(slots=(0, n_slots)), dict(slots=(-1, 1)),               # a slot outside 0..n_slots-1
        dict(pos=(5, C)), dict(pos=(-1, 100)),                       # a position outside 0..n_ctx-1
        dict(layer=n_layer), dict(layer=-1),                         # layer outside 0..n_layer-1
        dict(H=2),                                                   # head_dim 256
        dict(C_=96, kc_=kc96, vc_=vc96, pos=(5, 90)),                # n_ctx < 128
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            attn(**kw)
        with pytest.raises(RuntimeError):
            rope(**kw)
    with pytest.raises(RuntimeError):
        attn(slots=(), pos=(), q=empty_q)                            # n < 1
    with pytest.raises(RuntimeError):
        rope(slots=(), pos=(), x=empty_x)
    for qt in (0, 1, 4, -1):                                         # a bad type
        with pytest.raises(RuntimeError):
            attn(qt=qt)
    # n_ctx no multiple of 32
    kc130 = np.zeros((1, 1, 130 * E0), np.uint16)
    with pytest.raises(RuntimeError):
        attn(C_=130, kc_=kc130, vc_=kc130, slots=(0, 0), layer=0)
    with pytest.raises(RuntimeError):
        rope(C_=130, kc_=kc130, vc_=kc130, slots=(0, 0), layer=0)
    # valid calls afterwards
    got, blocks = attn()
    check_rows(oracle, got, blocks, oracle_rows(oracle, kc, vc, 1, q2, [0, 1], [5, 100], E0, H0, C), 2, [5, 100])
    q16, got_k, _ = rope()
    y = np.zeros(E0, np.float32)
    oracle.lib.orc_rope(np.ascontiguousarray(qkv2[1, :E0]), 128, H0, 1, 100, y)
    assert np.array_equal(q16[1], f16_bits(oracle, y))
    oracle.lib.orc_rope(np.ascontiguousarray(qkv2[1, E0:2 * E0]), 128, H0, 1, 100, y)
    assert np.array_equal(got_k[1, 1].reshape(C, E0)[100], f16_bits(oracle, y))


# ---- (h) the fused Wo quantizers of the single-sequence attention kernels

@pytest.mark.parametrize("kind,n_past,N,C", [(0, 200, 1, 256), (1, 200, 1, 256), (2, 200, 1, 256),
                                             (0, 60, 37, 256), (1, 60, 37, 256),
                                             (0, 700, 1, 1024), (2, 700, 1, 1024)])
@pytest.mark.parametrize("qt", [2, 3])
def test_attention_quantized_output(lvk, oracle, qt, kind, n_past, N, C):
    """attention.hip (kind 0), attention_prompt.hip (1) and attention_decode.hip (2): the f32 rows
    against orc_attention and the quantized Wo input against oracle.quantize of them, row by row,
    for both block types"""
    rng = np.random.default_rng(n_past * 13 + N + C)
    kc = rng.standard_normal(C * E0).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(C * E0).astype(np.float16).view(np.uint16).copy()
    q = rng.standard_normal(N * E0).astype(np.float32)
    want = np.zeros(N * E0, np.float32)
    oracle.lib.orc_attention(kc, vc, q, E0, H0, C, n_past, N, want)
    got, blocks = lvk.attention_q(kind, qt, kc, vc, q, E0, H0, C, n_past, N)
    check_rows(oracle, got, blocks, want.reshape(N, E0), qt, [n_past + t for t in range(N)])


def test_attention_quantized_output_bad_arguments(lvk):
    kc = np.zeros(256 * E0, np.uint16)
    q = np.zeros(2 * E0, np.float32)
    for kind, qt, C, n_past, N in [(3, 2, 256, 0, 1), (-1, 2, 256, 0, 1), (0, 4, 256, 0, 1), (0, 2, 256, 255, 2),
                                   (0, 2, 256, -1, 1), (2, 2, 256, 0, 2), (0, 2, 256, 0, 0)]:
        with pytest.raises(RuntimeError):
            lvk.attention_q(kind, qt, kc, kc, q[:N * E0], E0, H0, C, n_past, N)
