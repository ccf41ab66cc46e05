"""Batched decode over KV slots (lvk_seq_init / lvk_seq_copy / lvk_decode_batch, include/lvk_ops.h).

Row (token, seq, pos) of a call is defined as llama_eval(ctx', &token, 1, pos, .) on a context
whose cache holds sequence seq.  So the reference of a sequence is a separate plain lvk.Llama
context that evaluates the sequence's tokens one at a time with eval([tok], pos) -- the
single-token decode path the other suites pin to the oracle and the reference build -- and every
comparison is bit equality of the logits rows (uint32 views, no tolerance).
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


def check_rows(lg, am, want, what):
    """lg [n][V], am [n] of one decode_batch against the list of reference rows"""
    assert lg.shape[0] == len(want) and am.shape[0] == len(want)
    for i, w in enumerate(want):
        assert np.array_equal(bits(lg[i]), bits(w[-1])), "%s: row %d" % (what, i)
        assert int(am[i]) == int(np.argmax(lg[i])), "%s: argmax of row %d" % (what, i)


@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_q4_1", "tiny_f16", "tiny_f32"])
def test_rows_match_single_token_evals(lvk, oracle, models, name):
    """four sequences at start offsets 0, 29, 61 and 125, one row each per call for 8 calls:
    n_kv = pos + 1 crosses 32, 64 and 128, where the double tail of the P.V dot is empty on one
    side and one element long on the other; the sequence at offset 0 ends after 4 calls, so later
    calls carry fewer rows than there are slots.  The offsets are filled through the prompt path
    on slot 0 + seq_copy (slot 0 keeps the 125-token one)."""
    from oracle_lib import forced_tokens
    path = models[name]
    n_ctx, steps = 256, 8
    offs = [29, 61, 125, 0]                  # sequence s: slot (s + 1) % 4, i.e. 1, 2, 0, 3
    slots = [1, 2, 0, 3]
    n_steps = [steps, steps, steps, 4]
    toks = [forced_tokens(offs[s] + steps, seed=11 + s) for s in range(4)]
    m = lvk.Llama(path, n_ctx=n_ctx)
    assert m.seq_count() == 1
    m.seq_init(4)
    assert m.seq_count() == 4
    refs = [lvk.Llama(path, n_ctx=n_ctx) for _ in range(4)]
    for s in range(4):
        if offs[s]:
            m.eval(toks[s][:offs[s]], 0)
            if slots[s] != 0:
                m.seq_copy(slots[s], 0, offs[s])
            refs[s].eval(toks[s][:offs[s]], 0)
    assert [m.seq_tokens(slots[s]) for s in range(4)] == offs
    # the oracle follows the sequence that crosses n_kv = 32 (the Q4 types: it loads no others)
    om = oracle.model(path, n_ctx) if name in ("tiny_q4_0", "tiny_q4_1") else None
    if om is not None:
        om.eval(toks[0][:offs[0]], 0)
    for k in range(steps):
        live = [s for s in range(4) if k < n_steps[s]]
        pos = [offs[s] + k for s in live]
        lg, am = m.decode_batch([toks[s][offs[s] + k] for s in live], [slots[s] for s in live], pos, argmax=True)
        want = [refs[s].eval([toks[s][offs[s] + k]], offs[s] + k) for s in live]
        check_rows(lg, am, want, "%s step %d" % (name, k))
        if om is not None:
            assert np.array_equal(bits(lg[0]), bits(om.eval([toks[0][offs[0] + k]], offs[0] + k)[-1])), "oracle, step %d" % k
        for s in range(4):
            assert m.seq_tokens(slots[s]) == offs[s] + min(k + 1, n_steps[s])
    assert m.seq_tokens(4) == -1 and m.seq_tokens(-1) == -1
    for c in refs + [m]:
        c.close()
    if om is not None:
        om.close()


def test_several_rows_of_one_sequence(lvk, models):
    """five consecutive positions of sequence 1 in one call, interleaved with three rows of
    sequence 2, equal the sequential single evals; a rewind then overwrites"""
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    m = lvk.Llama(path, n_ctx=128)
    m.seq_init(3)
    r1, r2 = lvk.Llama(path, n_ctx=128), lvk.Llama(path, n_ctx=128)
    t1, t2 = forced_tokens(8, seed=21), forced_tokens(8, seed=22)
    order = [(1, 0), (2, 0), (1, 1), (2, 1), (1, 2), (1, 3), (2, 2), (1, 4)]     # (sequence, position)
    tok = [int((t1 if s == 1 else t2)[p]) for s, p in order]
    lg, am = m.decode_batch(tok, [s for s, _ in order], [p for _, p in order], argmax=True)
    want = [(r1 if s == 1 else r2).eval([t], p) for (s, p), t in zip(order, tok)]
    check_rows(lg, am, want, "interleaved")
    assert (m.seq_tokens(0), m.seq_tokens(1), m.seq_tokens(2)) == (0, 5, 3)
    # rewind sequence 1 to position 2 with another token, then go on from there
    lg, _ = m.decode_batch([int(t1[6])], [1], [2])
    assert np.array_equal(bits(lg[0]), bits(r1.eval([int(t1[6])], 2)[-1]))
    assert m.seq_tokens(1) == 3
    lg, _ = m.decode_batch([int(t1[7]), int(t2[3])], [1, 2], [3, 3])
    assert np.array_equal(bits(lg[0]), bits(r1.eval([int(t1[7])], 3)[-1]))
    assert np.array_equal(bits(lg[1]), bits(r2.eval([int(t2[3])], 3)[-1]))
    for c in (m, r1, r2):
        c.close()


def test_prefix_fanout_and_slot0_interop(lvk, models):
    """a prompt evaluated once on slot 0 fans out to slots 1 (all of it) and 2 (5 positions);
    batch steps on the three slots equal three contexts that evaluated the prompt themselves,
    and slot 0 then continues through the ordinary llama_eval (captured decode graph)"""
    path = models["tiny_q4_0"]
    m = lvk.Llama(path, n_ctx=128)
    kv_size = lvk.lib.llama_get_kv_cache_size(m.ctx)
    m.seq_init(3)
    m.eval(PROMPT, 0)
    n = len(PROMPT)
    assert m.seq_tokens(0) == n
    m.seq_copy(1, 0, n)
    m.seq_copy(2, 0, 5)
    refs = [lvk.Llama(path, n_ctx=128) for _ in range(3)]
    for r in refs:
        r.eval(PROMPT, 0)
    pos = [n, n, 5]
    tok = [[11, 22, 33], [44, 55, 66], [77, 88, 99]]      # per step: the tokens of slots 0, 1, 2
    for step in range(3):
        lg, am = m.decode_batch(tok[step], [0, 1, 2], [p + step for p in pos], argmax=True)
        want = [refs[s].eval([tok[step][s]], pos[s] + step) for s in range(3)]
        check_rows(lg, am, want, "step %d" % step)
    assert [m.seq_tokens(s) for s in range(3)] == [n + 3, n + 3, 8]
    assert m.kv_cache_token_count() == n + 3
    a = m.eval([123], n + 3)
    b = refs[0].eval([123], n + 3)
    assert np.array_equal(bits(a), bits(b))
    assert m.seq_tokens(0) == n + 4
    assert lvk.lib.llama_get_kv_cache_size(m.ctx) == kv_size
    for c in refs + [m]:
        c.close()


@pytest.mark.parametrize("ftype,n_big", [(2, 18), (3, 16)])
def test_7b_shaped_rows(lvk, model_dir, ftype, n_big):
    """7B layer shapes: (a) >= 16 rows, one per slot (the MFMA matmuls), (b) 3 rows (the multi-row
    matvec), positions spread over 20..140 so that the reference's decode attention runs both its
    short schedule and its score exchange.  The slots are copies of one 140-token prefix at
    different lengths, and the reference is one context holding the same prefix: a single-token
    eval at n_past = m reads only positions < m, so it serves every slot."""
    from oracle_lib import forced_tokens, gen_model
    if ftype == 2:
        path = gen_model(os.path.join(model_dir, "w4096_l2.bin"), n_embd=4096, n_head=32, n_layer=2, ftype=2, seed=7)
    else:     # the file of test_gpu_model.py's Q4_1 7B-shaped case
        path = gen_model(os.path.join(model_dir, "w4096_l2_q41.bin"), n_embd=4096, n_head=32, n_layer=2, ftype=3, seed=12)
    n_ctx, n_pre = 256, 140
    pre = forced_tokens(n_pre, seed=31)
    lens = [20 + (i * (n_pre - 20)) // (n_big - 1) for i in range(n_big)]        # 20 .. 140, ascending
    assert lens[0] == 20 and lens[-1] == n_pre and all(b - a >= 2 for a, b in zip(lens, lens[1:]))
    tok = forced_tokens(n_big, seed=32)        # (a): the row of slot 1 + i, at position lens[i]
    pick = [0, n_big // 2, n_big - 1]          # (b): these slots go one position further
    tok2 = forced_tokens(3, seed=33)
    checked = sorted({0, 1, 2, n_big // 2, n_big // 2 + 1, n_big - 2, n_big - 1})
    # the reference rows, longest slot first: the evals of slot i write positions >= lens[i] of the
    # one reference cache, which the shorter slots' evals after them never read
    r = lvk.Llama(path, n_ctx=n_ctx)
    r.eval(pre, 0)
    want_a, want_b = {}, {}
    for i in reversed(checked):
        want_a[i] = r.eval([int(tok[i])], lens[i])
        if i in pick:
            want_b[i] = r.eval([int(tok2[pick.index(i)])], lens[i] + 1)
    r.close()
    m = lvk.Llama(path, n_ctx=n_ctx)
    m.seq_init(n_big + 1)
    m.eval(pre, 0)
    for i, n in enumerate(lens):
        m.seq_copy(1 + i, 0, n)
    lg, am = m.decode_batch(tok, [1 + i for i in range(n_big)], lens, argmax=True)
    for i in checked:
        assert np.array_equal(bits(lg[i]), bits(want_a[i][-1])), "(a) row %d, n_past %d" % (i, lens[i])
    assert np.array_equal(am, np.argmax(lg, axis=1))
    lg, am = m.decode_batch(tok2, [1 + i for i in pick], [lens[i] + 1 for i in pick], argmax=True)
    for j, i in enumerate(pick):
        assert np.array_equal(bits(lg[j]), bits(want_b[i][-1])), "(b) row %d, n_past %d" % (j, lens[i] + 1)
    assert np.array_equal(am, np.argmax(lg, axis=1))
    assert [m.seq_tokens(1 + i) for i in range(n_big)] == [n + (2 if i in pick else 1) for i, n in enumerate(lens)]
    m.close()


@pytest.mark.parametrize("ftype", [2, 3])
def test_rows_past_512_positions_match_the_oracle(lvk, oracle, model_dir, ftype):
    """n_ctx = 1024 and slots of 500 .. 600 positions, one row each in one call: n_kv = pos + 1 of
    501, 512, 513, 531, 544, 545 and 601 runs the rows attention's second K block, its V steps
    from global memory and its double tail from LDS and from global memory, with the context's slot
    table, layer_off of the second layer at this n_ctx and lvk_seq_copy past 512 positions.  The
    slots are copies of one 600-token prefix evaluated through the prompt path; every logits row
    is compared with the oracle model, which evaluates the prefix once and then the single tokens
    longest slot first (as in test_7b_shaped_rows: an eval at n_past = m writes position m, which
    the evals of the shorter slots after it never read)."""
    from oracle_lib import forced_tokens, gen_model
    path = gen_model(os.path.join(model_dir, "w256_l2_t%d.bin" % ftype), n_embd=256, n_head=2, n_layer=2, ftype=ftype,
                     seed=40 + ftype)
    n_ctx, n_pre = 1024, 600
    lens = [500, 511, 512, 530, 543, 544, 600]
    pre = forced_tokens(n_pre, seed=41)
    tok = forced_tokens(len(lens), seed=42)
    om = oracle.model(path, n_ctx)
    om.eval(pre, 0)
    want = [None] * len(lens)
    for i in reversed(range(len(lens))):
        want[i] = om.eval([int(tok[i])], lens[i])
    om.close()
    m = lvk.Llama(path, n_ctx=n_ctx)
    m.seq_init(len(lens) + 1)
    m.eval(pre, 0)
    for i, n in enumerate(lens):
        m.seq_copy(1 + i, 0, n)
    assert [m.seq_tokens(1 + i) for i in range(len(lens))] == lens
    lg, am = m.decode_batch(tok, [1 + i for i in range(len(lens))], lens, argmax=True)
    check_rows(lg, am, want, "ftype %d" % ftype)
    assert [m.seq_tokens(1 + i) for i in range(len(lens))] == [n + 1 for n in lens]
    m.close()


def test_batch_errors(lvk, models):
    """argument checks: every bad call raises, changes no slot's count and leaves the context
    usable; contexts that cannot hold slots refuse seq_init and still evaluate"""
    path = models["tiny_q4_0"]
    n_ctx = 128
    m = lvk.Llama(path, n_ctx=n_ctx)
    r = lvk.Llama(path, n_ctx=n_ctx)
    m.seq_init(3)
    m.seq_init(2)                             # smaller: a no-op
    assert m.seq_count() == 3
    m.decode_batch([5, 6, 7], [1, 1, 2], [0, 1, 0])
    for t, p in ((5, 0), (6, 1)):
        r.eval([t], p)
    counts = [0, 2, 1]
    bad = [
        ([5], [3], [0]),                      # seq id >= seq_count
        ([5], [-1], [0]),
        ([5], [1], [n_ctx]),                  # pos >= n_ctx
        ([5], [1], [-1]),
        ([5], [1], [3]),                      # a hole: pos > the slot's count
        ([5, 6], [1, 1], [0, 2]),             # rows of one sequence at non-consecutive positions
        ([5, 6], [1, 1], [1, 0]),
        ([32000], [1], [2]),                  # token id out of range
        ([-1], [1], [2]),
        ([], [], []),                         # n = 0
        ([5] * (n_ctx + 1), [1] * (n_ctx + 1), list(range(n_ctx + 1))),     # n > n_ctx
    ]
    for tok, seq, pos in bad:
        with pytest.raises(RuntimeError):
            m.decode_batch(tok, seq, pos)
        assert [m.seq_tokens(s) for s in range(3)] == counts
    with pytest.raises(RuntimeError):
        m.seq_copy(3, 0, 0)                   # bad slot id
    with pytest.raises(RuntimeError):
        m.seq_copy(2, 1, 3)                   # more than the source holds
    assert [m.seq_tokens(s) for s in range(3)] == counts
    lg, _ = m.decode_batch([9], [1], [2])
    assert np.array_equal(bits(lg[0]), bits(r.eval([9], 2)[-1]))
    assert m.seq_tokens(1) == 3
    with pytest.raises(RuntimeError):
        m.seq_init(0)
    m.close()
    # a layer split and the f32 KV cache refuse slots and go on evaluating
    want = r.eval(PROMPT, 0)
    for kw in (dict(split=[0, 0], transport="copy"), dict(f16_kv=False)):
        c = lvk.Llama(path, n_ctx=n_ctx, **kw)
        with pytest.raises(RuntimeError):
            c.seq_init(2)
        assert c.seq_count() == 1
        with pytest.raises(RuntimeError):
            c.decode_batch([5], [0], [0])
        got = c.eval(PROMPT, 0)
        if "split" in kw:
            assert np.array_equal(bits(got), bits(want))
        else:
            assert np.all(np.isfinite(got))
        c.close()
    r.close()
