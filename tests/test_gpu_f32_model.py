"""f32 model files (every tensor ggml type 0) through the drop-in llama.h API on the GPU.

The tiny seeded f32 model (tests/golden/make_golden_f32.py) is compared bit-for-bit with the
logits the reference build produced (committed golden) and with the reference build live
(`ref`).  The reference loader only accepts 32 / 40 / 60 / 80 layers (llama.cpp:741-749), so
the 7B / 13B-shaped single-layer files cannot be loaded by it: there the batched matmul path (the f32
matrix cores) and the decode matvec path are checked against each other end to end (the
reference's result does not depend on the batching), each kernel being pinned to
ggml_vec_dot_f32 at those row lengths by tests/test_gpu_f32_ops.py.
"""
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden_f32 import CFG, NAME, logits_from_planes  # noqa: E402

PROMPT = np.array([1, 450, 4996, 17354, 1701, 29916, 338, 263, 3081, 310, 278, 2343], np.int32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.fixture(scope="module")
def tiny_f32(model_dir):
    from oracle_lib import gen_model
    return gen_model(os.path.join(model_dir, NAME + ".bin"), **CFG)


@pytest.mark.parametrize("graph", [True, False])
def test_tiny_f32_matches_reference_golden(lvk, tiny_f32, graph):
    g = np.load(os.path.join(GOLD, NAME + ".npz"), allow_pickle=False)
    want = logits_from_planes(g["logits_planes"])
    m = lvk.Llama(tiny_f32, n_ctx=512)
    m.set_graph(graph)
    n_past, off = 0, 0
    for step, n in enumerate(g["chunks"]):
        lg = m.eval(g["tokens"][off:off + n], n_past)
        assert np.array_equal(bits(lg[-1]), bits(want[step])), "step %d (n=%d, n_past=%d)" % (step, n, n_past)
        n_past += n
        off += n
    m.close()


@pytest.mark.parametrize("f16_kv", [True, False])
def test_tiny_f32_long_decode_vs_ref(lvk, ref, tiny_f32, f16_kv):
    """prompt chunks 16, 8, 24, then 130 decode steps: across the attention kernels' n_kv
    32 / 64 / 128 boundaries, with the f16 and the f32 KV cache"""
    from oracle_lib import prompt_tokens
    m = lvk.Llama(tiny_f32, n_ctx=256, f16_kv=f16_kv)
    rm = ref.model(tiny_f32, 256, f16_kv=f16_kv)
    toks = prompt_tokens(48)
    n_past = 0
    for ch in (16, 8, 24):
        a = m.eval(toks[n_past:n_past + ch], n_past)
        b = rm.eval(toks[n_past:n_past + ch], n_past)
        assert np.array_equal(bits(a), bits(b)), "chunk at n_past %d" % n_past
        n_past += ch
    tok = int(np.argmax(a[-1]))
    bad = []
    for _ in range(130):
        a = m.eval([tok], n_past)
        b = rm.eval([tok], n_past)
        if not np.array_equal(bits(a), bits(b)):
            bad.append(n_past)
        n_past += 1
        tok = int(np.argmax(b[-1]))
    assert not bad, "n_past %s" % bad[:20]
    m.close()
    rm.close()


def test_tiny_f32_logits_all_vs_ref(lvk, ref, tiny_f32):
    m = lvk.Llama(tiny_f32, n_ctx=128, logits_all=True, embedding=True)
    rm = ref.model(tiny_f32, 128, logits_all=True)
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, 40)], np.int32)
    a = m.eval(toks, 0)
    b = rm.eval(toks, 0)
    assert a.shape == b.shape == (40, m.n_vocab)
    assert np.array_equal(bits(a), bits(b))
    e = m.embeddings()
    assert e.shape == (m.n_embd,) and np.isfinite(e).all()
    m.close()
    rm.close()


@pytest.mark.parametrize("cfg,n2,steps", [(dict(n_embd=4096, n_head=32, seed=21), 24, 12),
                                          (dict(n_embd=5120, n_head=40, seed=22), 20, 8)], ids=["7b", "13b"])
def test_shaped_one_layer_batched_equals_decode(lvk, model_dir, cfg, n2, steps):
    """LLaMA-7B / 13B layer shapes (K = 4096 / 11008, 5120 / 13824), one layer, ftype 0: an
    8-token prompt (half a token tile), an n2-token prompt, then greedy decode steps; the same
    tokens fed one at a time through the decode matvec give the same logits bits at every
    compared position (see the module docstring for why not `ref`)"""
    from oracle_lib import gen_model, prompt_tokens
    path = gen_model(os.path.join(model_dir, "w%d_l1_f32.bin" % cfg["n_embd"]), n_layer=1, ftype=0, **cfg)
    m = lvk.Llama(path, n_ctx=128)
    toks = prompt_tokens(8 + n2)
    rows = [m.eval(toks[:8], 0)[-1].copy(), m.eval(toks[8:], 8)[-1].copy()]
    assert np.isfinite(rows[0]).all() and np.ptp(rows[0]) > 0
    fed = list(toks)
    tok, n_past = int(np.argmax(rows[-1])), len(toks)
    for _ in range(steps):
        fed.append(tok)
        rows.append(m.eval([tok], n_past)[-1].copy())
        n_past += 1
        tok = int(np.argmax(rows[-1]))
    # again from position 0, one token per eval
    check = {7: 0, len(toks) - 1: 1}
    for i in range(steps):
        check[len(toks) + i] = 2 + i
    for pos, t in enumerate(fed):
        lg = m.eval([int(t)], pos)[-1]
        if pos in check:
            assert np.array_equal(bits(lg), bits(rows[check[pos]])), "position %d" % pos
    m.close()


def test_tiny_f32_device_decode_paths(lvk, tiny_f32):
    """decode_chain with digests over 32 teacher-forced steps equals the per-step eval logits
    digests and argmaxes; eval_greedy equals the argmax of eval"""
    from oracle_lib import forced_tokens
    m = lvk.Llama(tiny_f32, n_ctx=128)
    m.eval(PROMPT, 0)
    seq = forced_tokens(32, seed=11)
    want_d, want_a = [], []
    for i in range(32):
        row = m.eval([int(seq[i])], len(PROMPT) + i)[-1]
        want_d.append(lvk.logits_digest(row))
        want_a.append(int(np.argmax(row)))
    m.eval(PROMPT, 0)
    got, dg = m.decode_chain(seq, len(PROMPT))
    assert dg.tolist() == want_d
    assert got.tolist() == want_a
    m.eval(PROMPT, 0)
    for i in range(6):
        assert m.eval_greedy(int(seq[i]), len(PROMPT) + i) == want_a[i]
    m.close()


def _run(m, steps):
    rows = [m.eval(PROMPT, 0)[-1].copy()]
    tok, n_past = int(np.argmax(rows[-1])), len(PROMPT)
    for _ in range(steps):
        rows.append(m.eval([tok], n_past)[-1].copy())
        n_past += 1
        tok = int(np.argmax(rows[-1]))
    return np.stack(rows)


def test_tiny_f32_split_and_stages(lvk, tiny_f32):
    ref = lvk.Llama(tiny_f32, n_ctx=128)
    want = _run(ref, 8)
    ref.close()
    m = lvk.Llama(tiny_f32, n_ctx=128, split=[0, 0], transport="copy")
    got = _run(m, 8)
    m.close()
    assert np.array_equal(bits(got), bits(want))
    # two stages handing the residual stream over through host memory
    L = CFG["n_layer"]
    s0 = lvk.Llama(tiny_f32, n_ctx=128, layers=(0, L // 2))
    s1 = lvk.Llama(tiny_f32, n_ctx=128, layers=(L // 2, L))
    buf = np.zeros((len(PROMPT), s0.n_embd), np.float32)

    def step(tokens, n_past):
        n = len(tokens)
        s0.stage_eval(np.asarray(tokens, np.int32), n, n_past)
        s0.get_x(buf.ctypes.data, n, False)
        s1.set_x(buf.ctypes.data, n, False)
        s1.stage_eval(None, n, n_past)
        return s1.logits()[-1].copy()

    rows = [step(PROMPT, 0)]
    tok, n_past = int(np.argmax(rows[-1])), len(PROMPT)
    for _ in range(8):
        rows.append(step([tok], n_past))
        n_past += 1
        tok = int(np.argmax(rows[-1]))
    s0.close()
    s1.close()
    assert np.array_equal(bits(np.stack(rows)), bits(want))


def test_tiny_f32_kv_cache_roundtrip(lvk, tiny_f32):
    m = lvk.Llama(tiny_f32, n_ctx=128)
    toks = np.arange(1, 20, dtype=np.int32)
    m.eval(toks, 0)
    kv = m.kv_cache()
    a = m.eval([42], 19)
    m2 = lvk.Llama(tiny_f32, n_ctx=128)
    m2.set_kv_cache(kv, 19)
    b = m2.eval([42], 19)
    assert np.array_equal(bits(a), bits(b))
    m.close()
    m2.close()


def test_tiny_f32_weight_bytes(lvk, tiny_f32):
    hp = lvk.model_hparams(tiny_f32)
    E, V, L = hp["n_embd"], hp["n_vocab"], hp["n_layer"]
    F = ((2 * (4 * E) // 3 + hp["n_mult"] - 1) // hp["n_mult"]) * hp["n_mult"]
    m = lvk.Llama(tiny_f32, n_ctx=128)
    assert m.weight_bytes() == 4 * (V * E + L * (4 * E * E + 3 * E * F))     # lm_head + the layer matrices
    assert m.prompt_image_bytes() == 0
    m.close()


def test_mixed_f32_f16_file_is_refused(lvk, tiny_f32, tmp_path):
    """one matrix switched to f16 among f32 ones: llama_init_from_file fails, no crash"""
    data = open(tiny_f32, "rb").read()
    n_vocab = struct.unpack_from("<I", data, 8)[0]
    off = 36
    for _ in range(n_vocab):
        off += 4 + struct.unpack_from("<I", data, off)[0] + 4
    out = bytearray(data[:off])
    switched = False
    while off < len(data):
        nd, nl, ft = struct.unpack_from("<III", data, off)
        assert ft == 0
        ne = struct.unpack_from("<%dI" % nd, data, off + 12)
        name_off = off + 12 + 4 * nd
        name = data[name_off:name_off + nl].decode()
        d = name_off + nl
        d += (32 - d % 32) % 32
        size = 4 * ne[0] * (ne[1] if nd > 1 else 1)
        rec = bytearray(data[off:d])
        if name == "layers.1.attention.wo.weight":
            struct.pack_into("<I", rec, 8, 1)
            out += rec + np.frombuffer(data, np.float32, ne[0] * ne[1], d).astype(np.float16).tobytes()   # a multiple of 32 bytes: alignment holds
            switched = True
        else:
            out += rec + data[d:d + size]
        off = d + size
    assert switched
    path = tmp_path / "mixed.bin"
    path.write_bytes(out)
    with pytest.raises(RuntimeError):
        lvk.Llama(str(path), n_ctx=64)
    m = lvk.Llama(tiny_f32, n_ctx=64)      # the library still loads the good file
    m.close()


def _tensors(data):
    """(vocab section end, [(name, dims, data bytes)]) of a single-part ggjt file of f32 tensors"""
    off = 36
    for _ in range(struct.unpack_from("<I", data, 8)[0]):
        off += 4 + struct.unpack_from("<I", data, off)[0] + 4
    vocab_end, out = off, []
    while off < len(data):
        nd, nl, ft = struct.unpack_from("<III", data, off)
        assert ft == 0
        ne = struct.unpack_from("<%dI" % nd, data, off + 12)
        name_off = off + 12 + 4 * nd
        d = name_off + nl
        d += (32 - d % 32) % 32
        size = 4 * ne[0] * (ne[1] if nd > 1 else 1)
        out.append((data[name_off:name_off + nl], ne, data[d:d + size]))
        off = d + size
    return vocab_end, out


@pytest.mark.parametrize("magic", [0x67676d66, 0x67676d6c], ids=["ggmf", "ggml"])
def test_tiny_f32_two_part_old_containers(lvk, tiny_f32, tmp_path, magic):
    """the tiny model rewritten as a two-part ggmf (versioned, vocab scores, no alignment) or
    ggml (unversioned, no scores) file: tok_embeddings, wo and w2 split by columns, the other
    matrices by rows (llama.cpp:533-540, 590-640); the 4-byte rows rejoin to the same model"""
    data = open(tiny_f32, "rb").read()
    vocab_end, tensors = _tensors(data)
    hdr = struct.pack("<I", magic) + (struct.pack("<I", 1) if magic == 0x67676d66 else b"") + data[8:36]
    if magic == 0x67676d66:
        hdr += data[36:vocab_end]
    else:                                   # ggml: the vocab entries carry no score
        off = 36
        while off < vocab_end:
            n = struct.unpack_from("<I", data, off)[0]
            hdr += data[off:off + 4 + n]
            off += 4 + n + 4
    by_cols = (b"tok_embeddings.", b".attention.wo.weight", b".feed_forward.w2.weight")
    parts = [bytearray(hdr), bytearray(hdr)]
    for name, ne, raw in tensors:
        for p in range(2):
            if len(ne) == 1:
                dims, piece = ne, raw
            else:
                w = np.frombuffer(raw, np.uint32).reshape(ne[1], ne[0])
                if any(k in name for k in by_cols):
                    dims, piece = (ne[0] // 2, ne[1]), np.ascontiguousarray(w[:, p * ne[0] // 2:(p + 1) * ne[0] // 2]).tobytes()
                else:
                    dims, piece = (ne[0], ne[1] // 2), w[p * ne[1] // 2:(p + 1) * ne[1] // 2].tobytes()
            parts[p] += struct.pack("<III", len(dims), len(name), 0) + struct.pack("<%dI" % len(dims), *dims) + name + piece
    path = tmp_path / "two.bin"
    path.write_bytes(parts[0])
    (tmp_path / "two.bin.1").write_bytes(parts[1])
    one = lvk.Llama(tiny_f32, n_ctx=128)
    want = _run(one, 4)
    one.close()
    two = lvk.Llama(str(path), n_ctx=128)
    got = _run(two, 4)
    two.close()
    assert np.array_equal(bits(got), bits(want))
