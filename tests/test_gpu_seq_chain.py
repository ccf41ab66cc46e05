"""Chained batched decode (lvk_decode_batch_chain, include/lvk_ops.h): n_steps steps of n rows, one
row per KV slot, in one call, the next tokens chosen on the device (forced or argmax).

Step i of row r is defined as llama_eval(ctx', &t_i[r], 1, pos[r] + i, .) on a context whose cache
holds sequence seqs[r].  The references are therefore plain lvk.Llama contexts on the single-token
paths the other suites pin (eval, decode_chain) or the host-fed decode_batch loop the chain
replaces, and every comparison is bit equality: uint32 views of logits, digests and tokens as
integers.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden_f16 import CFG as CFG_F16, NAME as NAME_F16  # noqa: E402
from make_golden_f32 import CFG as CFG_F32, NAME as NAME_F32  # noqa: E402

PROMPT = np.array([1, 450, 4996, 17354, 1701, 29916, 338, 263], np.int32)
N_CTX = 256
OFFS = [29, 61, 0]        # sequence s starts at OFFS[s] on slot SLOTS[s]
SLOTS = [1, 2, 0]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.fixture(scope="module")
def models(tiny_models, model_dir):
    from oracle_lib import gen_model
    d = dict(tiny_models)
    d["tiny_f16"] = gen_model(os.path.join(model_dir, NAME_F16 + ".bin"), **CFG_F16)
    d["tiny_f32"] = gen_model(os.path.join(model_dir, NAME_F32 + ".bin"), **CFG_F32)
    return d


def seq_prefixes(seed0, extra):
    """the three sequences' tokens: OFFS[s] prefix tokens, then `extra` more"""
    from oracle_lib import forced_tokens
    return [forced_tokens(OFFS[s] + extra, seed=seed0 + s) for s in range(3)]


def three_slots(lvk, path, toks):
    """a context whose slots 1, 2, 0 hold the sequences' prefixes (29, 61 and 0 positions: slot 0
    is emptied after it served as the staging slot), and one reference context per sequence"""
    m = lvk.Llama(path, n_ctx=N_CTX)
    m.seq_init(3)
    refs = [lvk.Llama(path, n_ctx=N_CTX) for _ in range(3)]
    for s in range(3):
        if OFFS[s]:
            m.eval(toks[s][:OFFS[s]], 0)
            m.seq_copy(SLOTS[s], 0, OFFS[s])
            refs[s].eval(toks[s][:OFFS[s]], 0)
    m.seq_copy(0, 0, 0)
    assert [m.seq_tokens(SLOTS[s]) for s in range(3)] == OFFS
    return m, refs


def host_loop(lvk, h, forced, seqs, pos, n_steps):
    """the loop the chain replaces: decode_batch per step, next tokens from the forced table, then
    from the step's device argmax.  Returns (tokens, digests, last logits)."""
    f = np.asarray(forced, np.int32).reshape(-1, len(seqs))
    tok, toks, dgs, lg = f[0], [], [], None
    for i in range(n_steps):
        lg, am = h.decode_batch(tok, seqs, [p + i for p in pos], argmax=True)
        toks.append(am.copy())
        dgs.append([lvk.logits_digest(row) for row in lg])
        tok = f[i + 1] if i + 1 < len(f) else am
    return np.array(toks, np.int32), np.array(dgs, np.uint64), lg


@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_q4_1", "tiny_f16", "tiny_f32"])
def test_forced_chain_matches_single_token_evals(lvk, models, name):
    """6 teacher-forced steps of three rows starting at 29, 61 (n_kv crosses 32 and 64 inside the
    call) and 0 (an empty slot): tokens, digests, the last logits, the counts and the KV contents
    (one further decode_batch step) against per-step evals on one context per sequence"""
    steps = 6
    toks = seq_prefixes(41, steps)
    m, refs = three_slots(lvk, models[name], toks)
    forced = np.array([[toks[s][OFFS[s] + i] for s in range(3)] for i in range(steps)], np.int32)
    got, dg, lg = m.decode_batch_chain(forced, SLOTS, OFFS, steps, digests=True, logits=True)
    assert got.shape == (steps, 3) and dg.shape == (steps, 3) and lg.shape == (3, m.n_vocab)
    for s in range(3):
        for i in range(steps):
            row = refs[s].eval([int(forced[i][s])], OFFS[s] + i)[-1]
            assert int(got[i][s]) == int(np.argmax(row)), "%s: token of row %d, step %d" % (name, s, i)
            assert int(dg[i][s]) == lvk.logits_digest(row), "%s: digest of row %d, step %d" % (name, s, i)
        assert np.array_equal(bits(lg[s]), bits(row)), "%s: last logits of row %d" % (name, s)
    assert [m.seq_tokens(SLOTS[s]) for s in range(3)] == [o + steps for o in OFFS]
    assert m.kv_cache_token_count() == steps
    nxt = [17, 2222, 31999]
    lg, _ = m.decode_batch(nxt, SLOTS, [o + steps for o in OFFS])
    for s in range(3):
        assert np.array_equal(bits(lg[s]), bits(refs[s].eval([nxt[s]], OFFS[s] + steps)[-1])), "%s: KV of row %d" % (name, s)
    for c in refs + [m]:
        c.close()


@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_f16"])
@pytest.mark.parametrize("n_forced", [1, 3])
def test_greedy_and_mixed_match_decode_chain(lvk, models, name, n_forced):
    """8 steps, greedy after 1 or 3 forced tokens: every row equals lvk_decode_chain on a context
    of its own holding that sequence, and the rows' greedy streams are not all the same one"""
    steps = 8
    toks = seq_prefixes(51, n_forced)
    m, refs = three_slots(lvk, models[name], toks)
    forced = np.array([[toks[s][OFFS[s] + i] for s in range(3)] for i in range(n_forced)], np.int32)
    # the Q4_0 file's greedy stream settles on one token after almost every input; after these
    # last forced tokens of the row at offset 0 it does not (found with the single-sequence path)
    forced[n_forced - 1][2] = {1: 14841, 3: 15797}[n_forced]
    got, dg, _ = m.decode_batch_chain(forced if n_forced > 1 else forced[0], SLOTS, OFFS, steps, digests=True)
    for s in range(3):
        want, want_d = refs[s].decode_chain(forced[:, s], OFFS[s], steps)
        assert got[:, s].tolist() == want.tolist(), "%s: tokens of row %d" % (name, s)
        assert dg[:, s].tolist() == want_d.tolist(), "%s: digests of row %d" % (name, s)
    greedy = got[n_forced - 1:]
    assert any(greedy[:, a].tolist() != greedy[:, b].tolist() for a, b in ((0, 1), (0, 2), (1, 2))), greedy
    assert [m.seq_tokens(SLOTS[s]) for s in range(3)] == [o + steps for o in OFFS]
    for c in refs + [m]:
        c.close()


def test_7b_shaped_rows_chain(lvk, model_dir):
    """7B layer shapes, slots copied from one 140-token prefix at lengths over 20..140: 16 rows
    (the MFMA matmuls) and 3 rows (the multi-row matvec), 4 steps with 2 forced, against a second
    context fed by the host through decode_batch"""
    from oracle_lib import forced_tokens, gen_model
    path = gen_model(os.path.join(model_dir, "w4096_l2.bin"), n_embd=4096, n_head=32, n_layer=2, ftype=2, seed=7)
    n_big, n_pre, steps = 16, 140, 4
    pre = forced_tokens(n_pre, seed=31)
    lens = [20 + (i * (n_pre - 20)) // (n_big - 1) for i in range(n_big)]
    ctxs = []
    for _ in range(2):
        c = lvk.Llama(path, n_ctx=N_CTX)
        c.seq_init(n_big + 1)
        c.eval(pre, 0)
        for i, n in enumerate(lens):
            c.seq_copy(1 + i, 0, n)
        ctxs.append(c)
    m, h = ctxs
    pick = [0, n_big // 2, n_big - 1]
    cases = [([1 + i for i in range(n_big)], lens, 61), ([1 + i for i in pick], [lens[i] for i in pick], 62)]
    for seqs, pos, seed in cases:
        n = len(seqs)
        forced = forced_tokens(2 * n, seed=seed).reshape(2, n)
        got, dg, lg = m.decode_batch_chain(forced, seqs, pos, steps, digests=True, logits=True)
        want, want_d, want_lg = host_loop(lvk, h, forced, seqs, pos, steps)
        assert np.array_equal(got, want), "%d rows: tokens" % n
        assert np.array_equal(dg, want_d), "%d rows: digests" % n
        assert np.array_equal(bits(lg), bits(want_lg)), "%d rows: last logits" % n
        assert [m.seq_tokens(s) for s in seqs] == [p + steps for p in pos]
    m.close()
    h.close()


def test_row_count_change_seq_init_and_graph_off(lvk, models):
    """calls with 3, 2 and 3 rows on one context (the step graph is rebuilt for another row
    count), a seq_init that grows the slot table between two calls (the graph holds the old
    table), then the same calls with the graph off (the launches enqueued eagerly): all equal the
    host-fed loop on a second context"""
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    m, h = lvk.Llama(path, n_ctx=128), lvk.Llama(path, n_ctx=128)
    for c in (m, h):
        c.seq_init(3)
    count = {s: 0 for s in range(5)}
    seed = [70]

    def call(seqs, steps, n_forced):
        n = len(seqs)
        seed[0] += 1
        forced = forced_tokens(n_forced * n, seed=seed[0]).reshape(n_forced, n)
        pos = [count[s] for s in seqs]
        got, dg, lg = m.decode_batch_chain(forced, seqs, pos, steps, digests=True, logits=True)
        want, want_d, want_lg = host_loop(lvk, h, forced, seqs, pos, steps)
        what = "call %d" % (seed[0] - 70)
        assert np.array_equal(got, want), what
        assert np.array_equal(dg, want_d), what
        assert np.array_equal(bits(lg), bits(want_lg)), what
        for s in seqs:
            count[s] += steps
        assert [m.seq_tokens(s) for s in range(m.seq_count())] == [count[s] for s in range(m.seq_count())]

    for graph in (1, 0):
        m.set_graph(graph)
        call([0, 1, 2], 5, 2)
        call([2, 1], 4, 1)
        call([1, 0, 2], 3, 3)
        if graph:
            for c in (m, h):
                c.seq_init(5)
            call([4, 2, 0], 4, 2)
            call([3], 3, 1)
    m.close()
    h.close()


def test_step_buffers_regrown_between_calls(lvk, models):
    """three calls of 3 rows on one context of n_ctx 128: 8 steps, then 60 (180 entries, past the
    first reserve of 128: the step outputs are replaced by larger buffers and the step graph, which
    held the old addresses, is captured again), then 8 on the grown buffers.  Tokens, digests and
    last logits of every call equal the host-fed loop on a second context"""
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    m, h = lvk.Llama(path, n_ctx=128), lvk.Llama(path, n_ctx=128)
    for c in (m, h):
        c.seq_init(3)
    seqs, pos = [0, 1, 2], [0, 0, 0]
    for k, steps in enumerate((8, 60, 8)):
        forced = forced_tokens(3, seed=90 + k).reshape(1, 3)
        got, dg, lg = m.decode_batch_chain(forced, seqs, pos, steps, digests=True, logits=True)
        want, want_d, want_lg = host_loop(lvk, h, forced, seqs, pos, steps)
        assert got.shape == (steps, 3), "call %d" % k
        assert np.array_equal(got, want), "call %d: tokens" % k
        assert np.array_equal(dg, want_d), "call %d: digests" % k
        assert np.array_equal(bits(lg), bits(want_lg)), "call %d: last logits" % k
        pos = [p + steps for p in pos]
        assert [m.seq_tokens(s) for s in seqs] == pos
    m.close()
    h.close()


def test_slot0_interop_and_default_context(lvk, models):
    """a chain that includes slot 0 leaves llama_get_kv_cache_token_count at its end, and the
    ordinary llama_eval continues from there; a context that never called seq_init chains on its
    one slot"""
    path = models["tiny_q4_0"]
    m, r = lvk.Llama(path, n_ctx=128), lvk.Llama(path, n_ctx=128)
    kv_size = lvk.lib.llama_get_kv_cache_size(m.ctx)
    n, steps = len(PROMPT), 4
    m.eval(PROMPT, 0)
    r.eval(PROMPT, 0)
    assert m.seq_count() == 1
    got, dg, _ = m.decode_batch_chain([77], [0], [n], steps, digests=True)       # no seq_init before it
    want, want_d = r.decode_chain([77], n, steps)
    assert got[:, 0].tolist() == want.tolist() and dg[:, 0].tolist() == want_d.tolist()
    assert m.seq_count() == 1 and m.kv_cache_token_count() == n + steps
    m.seq_init(2)
    m.seq_copy(1, 0, 5)
    got, _, _ = m.decode_batch_chain([88, 99], [0, 1], [n, 5], steps)             # slot 0 rewound to n
    want = r.decode_chain([88], n, steps, digests=False)
    assert got[:, 0].tolist() == want.tolist()
    assert m.kv_cache_token_count() == n + steps and m.seq_tokens(1) == 5 + steps
    a = m.eval([123], m.kv_cache_token_count())
    b = r.eval([123], n + steps)
    assert np.array_equal(bits(a), bits(b))
    assert m.seq_tokens(0) == n + steps + 1
    assert lvk.lib.llama_get_kv_cache_size(m.ctx) == kv_size
    m.close()
    r.close()


def test_rows_step_op(lvk):
    """the tail kernel alone on host rows of 32000 = 31 * 1024 + 256 logits: a duplicated maximum
    (first wins), a maximum in the tail past 31 * 1024, a NaN at index 0; the digests; the next
    token forced while step + 1 < n_forced"""
    V, n = 32000, 3
    rng = np.random.RandomState(9)
    x = rng.standard_normal((n, V)).astype(np.float32)
    x[0, 5] = x[0, V - 1] = 9.0
    x[1, V - 1] = 9.0
    x[2, 0] = np.nan
    x[2, 777] = 9.0
    forced = np.array([[10, 11, 12], [20, 21, 22], [30, 31, 32]], np.int32)
    want_d = [lvk.logits_digest(row) for row in x]
    for step, want_next in ((0, [20, 21, 22]), (1, [30, 31, 32]), (2, [5, V - 1, 0]), (7, [5, V - 1, 0])):
        am, dg, nt = lvk.rows_step(x, forced, step)
        assert am.tolist() == [5, V - 1, 0], step
        assert dg.tolist() == want_d, step
        assert nt.tolist() == want_next, step
    am, _, nt = lvk.rows_step(x, None, 0)
    assert am.tolist() == [5, V - 1, 0] and nt.tolist() == [5, V - 1, 0]


def test_chain_errors(lvk, models):
    """every bad call raises, changes no slot's count and leaves the context able to run a correct
    decode_batch step; contexts that cannot hold slots refuse the chain and still evaluate"""
    path = models["tiny_q4_0"]
    n_ctx = 128
    m, r = lvk.Llama(path, n_ctx=n_ctx), lvk.Llama(path, n_ctx=n_ctx)
    m.seq_init(3)
    m.decode_batch([5, 6, 7], [1, 1, 2], [0, 1, 0])
    for t, p in ((5, 0), (6, 1)):
        r.eval([t], p)
    counts = [0, 2, 1]
    f1 = [[5, 6]]
    bad = [
        (f1, [1, 1], [0, 0], 2),                          # a slot named twice
        (f1, [1, 2], [3, 0], 2),                          # a hole: pos > the slot's count
        (f1, [1, 2], [2, 1], n_ctx - 1),                  # pos + n_steps > n_ctx
        ([[5]], [0], [0], n_ctx + 1),
        (f1, [1, 2], [2, 1], 0),                          # n_steps = 0
        (np.zeros((0, 2), np.int32), [1, 2], [2, 1], 2),  # n_forced = 0
        ([[5, 6]] * 3, [1, 2], [2, 1], 2),                # n_forced > n_steps
        ([[5, 6], [7, 32000]], [1, 2], [2, 1], 2),        # a forced token out of range in the last forced row
        ([[5, 6], [-1, 7]], [1, 2], [2, 1], 2),
        (f1, [1, 3], [2, 0], 2),                          # slot id out of range
        (f1, [-1, 2], [0, 1], 2),
        (f1, [1, 2], [-1, 1], 2),
        (np.zeros((1, 0), np.int32), [], [], 2),          # n = 0
    ]
    for forced, seqs, pos, steps in bad:
        with pytest.raises(RuntimeError):
            m.decode_batch_chain(forced, seqs, pos, steps, digests=True)
        assert [m.seq_tokens(s) for s in range(3)] == counts
    lg, _ = m.decode_batch([9], [1], [2])
    assert np.array_equal(bits(lg[0]), bits(r.eval([9], 2)[-1]))
    assert m.seq_tokens(1) == 3
    m.close()
    want = r.eval(PROMPT, 0)
    for kw in (dict(split=[0, 0], transport="copy"), dict(f16_kv=False)):
        c = lvk.Llama(path, n_ctx=n_ctx, **kw)
        with pytest.raises(RuntimeError):
            c.decode_batch_chain([5], [0], [0], 2)
        assert c.seq_count() == 1
        got = c.eval(PROMPT, 0)
        if "split" in kw:
            assert np.array_equal(bits(got), bits(want))
        else:
            assert np.all(np.isfinite(got))
        c.close()
    r.close()
