"""Batched decode that ends in the reference's sampler, per row (lvk_decode_batch_sample,
lvk_seq_seed, lvk_sample_fallbacks, lvk_sample_candidates_rows; include/lvk_ops.h).

Op level: the rows kernel (sample.hip, one workgroup per selected row) against a numpy restatement
of the values the reference sorts (llama.cpp:1398-1414) and against the single-row kernel.

Model level: row i of a call is llama_eval of one token on the row's sequence followed by
llama_sample_top_p_top_k drawing from the sequence's slot's generator.  So the reference of a
sequence is one separate plain context that replays the sequence alone: reseeded with
seq_seed(0, seed), prefilled token by token (the rows' definition is the single-token eval), then
eval_sample -- the single-sequence device sampler that test_gpu_sampling.py pins to the reference
build.  Every comparison is equality of token streams.

The assertions that no row took the all-logits path are conditions on the inputs: the prompts,
seeds and parameters below were checked on the CPU to have no two equal values among any step's
top-k candidates and the value after them -- with the reference build for the tiny models, and with
the CPU oracle's logits for the 2-layer 7B-shaped model, which the reference build does not load.
Such ties are not rare on these synthetic models (one in 128 sampled rows of another prompt set), so
a changed prompt wants that check again.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SP = dict(top_k=40, top_p=0.95, temp=0.8, repeat_penalty=1.1)
# per-row parameters of the three-sequence test
ROW_PARAMS = [SP, dict(top_k=5, top_p=0.5, temp=0.3, repeat_penalty=1.3), dict(top_k=1, top_p=0.9, temp=2.0, repeat_penalty=1.1)]
ROW_LENS = [6, 9, 13]
ROW_SEED, ROW_STEPS = 3, 24
BIG = dict(n_embd=4096, n_head=32, n_layer=2, ftype=2, seed=7)     # w4096_l2.bin, as test_gpu_sampling.py
BIG_SEQS, BIG_STEPS, BIG_SEED = 16, 8, 1
REGROW_SEQS, REGROW_SEED, REGROW_PROMPT_SEED = 20, 1, 170   # test_sampler_buffers_regrown_between_calls


def prompt(n, seed):
    from oracle_lib import forced_tokens
    return [1] + forced_tokens(n - 1, seed=seed).tolist()


def row_prompts():
    return [prompt(n, 130 + i) for i, n in enumerate(ROW_LENS)]


def big_prompts():
    return [prompt(3 + s % 3, 150 + s) for s in range(BIG_SEQS)]


def window(tokens):
    """main.cpp's last_n_tokens: 64 zeros, then the tokens"""
    return ([0] * 64 + [int(t) for t in tokens])[-64:]


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


# ---------------------------------------------------------------------------
# op level: lvk_sample_candidates_rows
# ---------------------------------------------------------------------------
def _ref_values(x, last, temp, rp):
    """the (value) array the reference sorts (llama.cpp:1398-1414), float32 ops in its order"""
    x = np.asarray(x, np.float32)
    scale = np.float32(1.0) / np.float32(temp)
    s = (x * scale).astype(np.float32)
    v = s.copy()
    inl = np.zeros(x.size, bool)
    for t in last:
        if 0 <= t < x.size:
            inl[t] = True
    neg = x < 0
    v[inl & neg] = (s[inl & neg] * np.float32(rp)).astype(np.float32)
    v[inl & ~neg] = (s[inl & ~neg] / np.float32(rp)).astype(np.float32)
    return v


def _pairs(vals, ids):
    """candidates in id order (the kernel's order is arbitrary): (ids, value bits)"""
    o = np.argsort(ids)
    return ids[o].tolist(), vals[o].view(np.uint32).tolist()


@pytest.mark.parametrize("n,ks,temps,rps,nls", [
    (7, [3], [0.5], [2.0], [3]),
    (1000, [1, 40, 1000], [1.0, 0.8, 1.0], [1.0, 1.1, 1.3], [0, 8, 1024]),
    (32000, [40, 1, 1024, 40, 5], [0.8, 2.0, 0.3, 1.5, 0.3], [1.1, 1.3, 1.1, 1.0, 1.3], [64, 0, 1024, 8, 3]),
], ids=["1x7", "3x1000", "5x32000"])
def test_rows_candidates_match_reference_values(lvk, n, ks, temps, rps, nls):
    """every row: the candidates are exactly the values >= the k-th largest of the reference's
    scaled / penalized values, bit-equal, with that row's own k, temp, rp and window"""
    rows = len(ks)
    rng = np.random.default_rng(n + rows)
    x = (rng.standard_normal((rows, n)) * 3).astype(np.float32)
    last = [rng.integers(0, n, nl).astype(np.int32) for nl in nls]
    got = lvk.sample_candidates_rows(x, list(range(rows)), ks, temps, rps, last)
    assert len(got) == rows
    for r, (vals, ids, flags, cnt) in enumerate(got):
        want = _ref_values(x[r], last[r], temps[r], rps[r])
        kth = np.sort(want)[::-1][ks[r] - 1]
        sel = np.nonzero(want >= kth)[0]
        assert flags == 0 and cnt == sel.size, "row %d" % r
        assert sorted(ids.tolist()) == sel.tolist(), "row %d" % r
        assert np.array_equal(vals.view(np.uint32), want[ids].view(np.uint32)), "row %d" % r


def test_rows_selected_by_row_index(lvk):
    """sel names rows of x, not launch indices: [4, 0, 2] of 5 rows gives those rows' candidates,
    each equal to the single-row kernel's on that row"""
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((5, 32000)) * 3).astype(np.float32)
    sel, ks, temps, rps = [4, 0, 2], [40, 7, 300], [0.8, 1.3, 0.5], [1.1, 1.0, 1.2]
    last = [rng.integers(0, 32000, nl).astype(np.int32) for nl in (64, 0, 500)]
    got = lvk.sample_candidates_rows(x, sel, ks, temps, rps, last)
    for j, r in enumerate(sel):
        vals, ids, flags, cnt = lvk.sample_candidates(x[r], last[j], ks[j], temps[j], rps[j])
        assert (got[j][2], got[j][3]) == (flags, cnt) == (0, cnt), "row %d" % r
        assert _pairs(got[j][0], got[j][1]) == _pairs(vals, ids), "row %d" % r


def test_rows_do_not_disturb_each_other(lvk):
    """one call, five rows: a NaN in row 1, a tie at row 2's k-th value and 1500 equal maxima in
    row 3 raise exactly their own rows' flags / counts; rows 0 and 4 equal their single-row results"""
    rng = np.random.default_rng(78)
    n, k = 32000, 40
    x = (rng.standard_normal((5, n)) * 3).astype(np.float32)
    x[1, 12345] = np.nan
    order = np.argsort(x[2])[::-1]
    x[2, order[k]] = x[2, order[k - 1]]           # the 41st equals the 40th
    x[3, rng.choice(n, 1500, replace=False)] = 50.0
    last = [rng.integers(0, n, 64).astype(np.int32) for _ in range(5)]
    last[2] = last[3] = np.zeros(0, np.int32)     # no penalty on the tied pair or the maxima
    got = lvk.sample_candidates_rows(x, [0, 1, 2, 3, 4], [k] * 5, [1.0] * 5, [1.1] * 5, last)
    assert [g[2] for g in got] == [0, 1, 0, 2, 0]
    assert got[2][3] == k + 1 and got[3][3] == 1500
    for r in (0, 4):
        vals, ids, flags, cnt = lvk.sample_candidates(x[r], last[r], k, 1.0, 1.1)
        assert flags == 0 and got[r][3] == cnt == k
        assert _pairs(got[r][0], got[r][1]) == _pairs(vals, ids)


def test_rows_bad_arguments(lvk):
    x = np.zeros((2, 100), np.float32)
    for sel, k, temp in (([2], [3], [1.0]), ([-1], [3], [1.0]), ([0], [0], [1.0]), ([0], [101], [1.0]), ([0], [3], [0.0])):
        with pytest.raises(RuntimeError):
            lvk.sample_candidates_rows(x, sel, k, temp, [1.0], [[]])
    with pytest.raises(RuntimeError):
        lvk.sample_candidates_rows(x, [0], [3], [1.0], [1.0], [list(range(1025))])


# ---------------------------------------------------------------------------
# model level: lvk_decode_batch_sample
# ---------------------------------------------------------------------------
def replay(r, seed, toks, sp, steps):
    """the stream of one sequence alone on context r: slot 0 reseeded, the tokens but the last
    evaluated one by one, then eval_sample from the last one on"""
    r.seq_seed(0, seed)
    for p, t in enumerate(toks[:-1]):
        r.eval([t], p)
    tok, n_past, last, out = int(toks[-1]), len(toks) - 1, window(toks), []
    for _ in range(steps):
        tok = r.eval_sample(tok, n_past, last, **sp)
        out.append(tok)
        last = last[1:] + [tok]
        n_past += 1
    return out


class Seqs:
    """the caller's side of a batched sampled decode: per sequence its slot, tokens so far and window"""

    def __init__(self, m, slots, prompts):
        self.m, self.slots = m, list(slots)
        self.toks = [[int(t) for t in p] for p in prompts]
        self.out = [[] for _ in prompts]
        t = [(tok, s, p) for s, pr in zip(self.slots, self.toks) for p, tok in enumerate(pr[:-1])]
        if t:     # every prompt token but the last, as plain rows
            m.decode_batch([a for a, _, _ in t], [b for _, b, _ in t], [c for _, _, c in t], logits=False)

    def step(self, sps, which=None):
        """one decode_batch_sample over the sequences `which` (default: all), each evaluating its
        last token"""
        which = list(range(len(self.slots))) if which is None else which
        got = self.m.decode_batch_sample([self.toks[i][-1] for i in which], [self.slots[i] for i in which],
                                         [len(self.toks[i]) - 1 for i in which],
                                         [dict(sps[i], last_tokens=window(self.toks[i])) for i in which])
        for i, t in zip(which, got.tolist()):
            assert 0 <= t < 32000
            self.toks[i].append(t)
            self.out[i].append(t)
        return got


@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_q4_1"])
def test_per_row_parameters_match_single_sequence_sampler(lvk, tiny_models, name):
    """three sequences with prompts of 6, 9 and 13 tokens and their own (top_k, top_p, temp,
    repeat_penalty), 24 sampled steps: every stream equals the sequence alone through eval_sample;
    no row took the all-logits path"""
    path = tiny_models[name]
    m = lvk.Llama(path, n_ctx=256, seed=ROW_SEED)
    m.seq_init(3)
    r = lvk.Llama(path, n_ctx=256, seed=99)
    prompts = row_prompts()
    sq = Seqs(m, [2, 0, 1], prompts)
    f0 = m.sample_fallbacks()
    for _ in range(ROW_STEPS):
        sq.step(ROW_PARAMS)
    assert m.sample_fallbacks() == f0 == 0
    for i, p in enumerate(prompts):
        assert sq.out[i] == replay(r, ROW_SEED, p, ROW_PARAMS[i], ROW_STEPS), "sequence %d" % i
    assert [m.seq_tokens(s) for s in (2, 0, 1)] == [n - 1 + ROW_STEPS for n in ROW_LENS]
    assert r.sample_fallbacks() == 0
    m.close()
    r.close()


def regrow_prompts():
    return [prompt(2 + s % 3, REGROW_PROMPT_SEED + s) for s in range(REGROW_SEQS)]


def test_sampler_buffers_regrown_between_calls(lvk, tiny_models):
    """three calls on one context: 2 device-sampled rows with 8-id windows, then 20 rows on 20
    slots with 64-id windows (past the first reserve of 16 rows and 1024 pool ints: the records,
    the candidates and the pool are replaced by larger buffers), then the first 2 rows again on
    the grown buffers.  Every token equals the sequence alone through eval_sample with the same
    seed, parameters and windows; no row took the all-logits path"""
    path = tiny_models["tiny_q4_0"]
    m = lvk.Llama(path, n_ctx=64, seed=REGROW_SEED)
    m.seq_init(REGROW_SEQS)
    r = lvk.Llama(path, n_ctx=64, seed=99)
    toks = regrow_prompts()
    pre = [(t, s, p) for s, pr in enumerate(toks) for p, t in enumerate(pr[:-1])]
    m.decode_batch([a for a, _, _ in pre], [b for _, b, _ in pre], [c for _, _, c in pre], logits=False)
    calls = [([0, 1], 8), (list(range(REGROW_SEQS)), 64), ([0, 1], 8)]
    out = [[] for _ in toks]
    for which, n_win in calls:
        got = m.decode_batch_sample([toks[i][-1] for i in which], which, [len(toks[i]) - 1 for i in which],
                                    [dict(SP, last_tokens=window(toks[i])[-n_win:]) for i in which])
        for i, t in zip(which, got.tolist()):
            toks[i].append(t)
            out[i].append(t)
    assert m.sample_fallbacks() == 0
    for i, p in enumerate(regrow_prompts()):
        # the sequence alone: slot 0 of r reseeded, the prompt token by token, then its draws
        r.seq_seed(0, REGROW_SEED)
        for pos, t in enumerate(p[:-1]):
            r.eval([t], pos)
        seq, want = list(p), []
        for which, n_win in calls:
            if i in which:
                want.append(r.eval_sample(seq[-1], len(seq) - 1, window(seq)[-n_win:], **SP))
                seq.append(want[-1])
        assert out[i] == want, "sequence %d" % i
    assert r.sample_fallbacks() == 0
    assert [m.seq_tokens(s) for s in range(REGROW_SEQS)] == [len(t) - 1 for t in toks]
    m.close()
    r.close()


def test_streams_match_reference_build(lvk, ref, tiny_models):
    """two sequences against two reference-build models (seed 1) fed token by token, slots
    reseeded to 1: 16 sampled steps give the reference's streams"""
    path = tiny_models["tiny_q4_0"]
    m = lvk.Llama(path, n_ctx=256, seed=8)
    m.seq_init(3)
    prompts = [prompt(7, 41), prompt(5, 42)]
    rs = [ref.model(path, 256) for _ in prompts]
    for s in (1, 2):
        m.seq_seed(s, 1)
    sq = Seqs(m, [1, 2], prompts)
    for _ in range(16):
        sq.step([SP, SP])
    for i, (r, p) in enumerate(zip(rs, prompts)):
        for pos, t in enumerate(p):
            r.eval([t], pos)
        toks, want = list(p), []
        for _ in range(16):
            t = r.sample(window(toks), SP["top_k"], SP["top_p"], SP["temp"], SP["repeat_penalty"])
            want.append(t)
            r.eval([t], len(toks))
            toks.append(t)
        assert sq.out[i] == want, "sequence %d" % i
        r.close()
    assert m.sample_fallbacks() == 0
    m.close()


def test_mixed_rows_in_one_call(lvk, tiny_models):
    """one call with two prefill rows (no token wanted), a greedy row, a device-path row and a
    top_k = 0 row: -1 for the prefill rows, decode_batch's argmax for the greedy one, exactly one
    all-logits row, and the greedy slot's generator untouched"""
    path = tiny_models["tiny_q4_0"]
    seed = 6
    m = lvk.Llama(path, n_ctx=256, seed=seed)
    m.seq_init(5)
    r = lvk.Llama(path, n_ctx=256, seed=99)
    pg, pd, ph, pp = prompt(5, 61), prompt(6, 62), prompt(4, 63), prompt(2, 64)
    sq = Seqs(m, [2, 3, 4], [pg, pd, ph])
    sps = [dict(SP, temp=0.0), SP, dict(SP, top_k=0)]
    tokens = [pp[0], pp[1], pg[-1], pd[-1], ph[-1]]
    seqs, pos = [1, 1, 2, 3, 4], [0, 1, len(pg) - 1, len(pd) - 1, len(ph) - 1]
    f0 = m.sample_fallbacks()
    got = m.decode_batch_sample(tokens, seqs, pos, [None, None] + [dict(sps[i], last_tokens=window(p))
                                                                   for i, p in enumerate((pg, pd, ph))])
    assert got[:2].tolist() == [-1, -1]
    assert m.sample_fallbacks() == f0 + 1
    assert [m.seq_tokens(s) for s in range(5)] == [0, 2, len(pg), len(pd), len(ph)]
    _, am = m.decode_batch(tokens, seqs, pos, logits=False, argmax=True)      # the same rows again (a rewind)
    assert int(got[2]) == int(am[2])
    assert int(got[3]) == replay(r, seed, pd, SP, 1)[0]
    assert int(got[4]) == replay(r, seed, ph, dict(SP, top_k=0), 1)[0]
    # the greedy row drew nothing: slot 2's next draws are a fresh generator's
    for i in range(3):
        sq.toks[i].append(int(got[2 + i]))
    for _ in range(6):
        sq.step([SP] * 3, which=[0])
    assert sq.out[0] == replay(r, seed, pg + [int(got[2])], SP, 6)
    m.close()
    r.close()


def test_slot0_draws_from_the_context_generator(lvk, tiny_models):
    """eval_sample and decode_batch_sample on slot 0, alternating, give the stream of a context
    that used eval_sample throughout"""
    path = tiny_models["tiny_q4_1"]
    a = lvk.Llama(path, n_ctx=256, seed=7)
    b = lvk.Llama(path, n_ctx=256, seed=7)
    p = prompt(6, 71)
    want = replay(b, 7, p, SP, 12)
    for pos, t in enumerate(p[:-1]):
        a.eval([t], pos)
    toks = list(p)
    for step in range(12):
        if step % 2:
            t = a.eval_sample(toks[-1], len(toks) - 1, window(toks), **SP)
        else:
            t = int(a.decode_batch_sample([toks[-1]], [0], [len(toks) - 1], [dict(SP, last_tokens=window(toks))])[0])
        toks.append(t)
    assert toks[len(p):] == want
    assert a.sample_fallbacks() == 0
    a.close()
    b.close()


def test_reseeding_a_slot_reproduces_its_stream(lvk, tiny_models):
    path = tiny_models["tiny_q4_0"]
    m = lvk.Llama(path, n_ctx=256, seed=5)
    m.seq_init(2)
    r = lvk.Llama(path, n_ctx=256, seed=99)
    p = prompt(8, 81)
    streams = []
    for _ in range(2):
        m.seq_seed(1, 11)
        sq = Seqs(m, [1], [p])           # starts again from position 0: a rewind
        for _ in range(12):
            sq.step([SP])
        streams.append(sq.out[0])
    assert streams[0] == streams[1] == replay(r, 11, p, SP, 12)
    with pytest.raises(RuntimeError):
        m.seq_seed(2, 1)
    m.close()
    r.close()


def _raw_call(lvk, m, tokens, seqs, pos, rows, out):
    arr = (lvk.lvk_row_sample * len(rows))(*rows)
    return lvk.lib.lvk_decode_batch_sample(m.ctx, np.asarray(tokens, np.int32), np.asarray(seqs, np.int32),
                                           np.asarray(pos, np.int32), len(tokens), C.addressof(arr),
                                           None if out is None else out.ctypes.data)


def test_argument_errors_change_nothing(lvk, tiny_models):
    """each bad call returns -1 and leaves every slot's count and every generator as it was: the
    streams sampled between the bad calls equal the replay that never saw them"""
    path = tiny_models["tiny_q4_0"]
    seed = 4
    m = lvk.Llama(path, n_ctx=256, seed=seed)
    m.seq_init(2)
    r = lvk.Llama(path, n_ctx=256, seed=99)
    prompts = [prompt(5, 91), prompt(7, 92)]
    sq = Seqs(m, [0, 1], prompts)
    win = np.asarray(window(prompts[0]), np.int32)
    out = np.zeros(2, np.int32)

    def row(n_last=64, last=win):
        return lvk.lvk_row_sample(1, 40, 0.95, 0.8, 1.1, n_last, None if last is None else last.ctypes.data)
    for case in ("n_last", "null_window", "seq_id", "hole", "null_out"):
        tokens = [sq.toks[0][-1], sq.toks[1][-1]]
        seqs, pos, rows, o = [0, 1], [len(sq.toks[0]) - 1, len(sq.toks[1]) - 1], [row(), row()], out
        if case == "n_last":
            rows[1] = row(n_last=-1)
        elif case == "null_window":
            rows[1] = row(n_last=3, last=None)
        elif case == "seq_id":
            seqs = [0, 2]
        elif case == "hole":
            pos = [pos[0], pos[1] + 1]
        else:
            o = None
        counts = [m.seq_tokens(0), m.seq_tokens(1)]
        assert _raw_call(lvk, m, tokens, seqs, pos, rows, o) == -1, case
        assert [m.seq_tokens(0), m.seq_tokens(1)] == counts, case
        for _ in range(2):
            sq.step([SP, SP])
    for i, p in enumerate(prompts):
        assert sq.out[i] == replay(r, seed, p, SP, 10), "sequence %d" % i
    m.close()
    r.close()


def test_f32_kv_context_refuses(lvk, tiny_models):
    m = lvk.Llama(tiny_models["tiny_q4_0"], n_ctx=64, f16_kv=False)
    with pytest.raises(RuntimeError):
        m.decode_batch_sample([1], [0], [0], [dict(SP)])
    assert m.seq_tokens(0) == 0 and m.sample_fallbacks() == 0
    assert m.eval([1], 0).shape == (1, 32000)               # the context still works
    m.close()


def test_7b_shaped_16_sequences(lvk, model_dir):
    """n_embd 4096, 2 layers, n_vocab 32000: 16 sequences sampled for 8 steps in one context --
    16 workgroups, row indices 0..15 at the real vocabulary size -- equal their single-sequence
    streams; no row took the all-logits path"""
    from oracle_lib import gen_model
    path = gen_model(os.path.join(model_dir, "w4096_l2.bin"), **BIG)
    m = lvk.Llama(path, n_ctx=64, seed=BIG_SEED)
    m.seq_init(BIG_SEQS)
    r = lvk.Llama(path, n_ctx=64, seed=99)
    prompts = big_prompts()
    slots = [(s + 5) % BIG_SEQS for s in range(BIG_SEQS)]
    sq = Seqs(m, slots, prompts)
    for _ in range(BIG_STEPS):
        sq.step([SP] * BIG_SEQS)
    assert m.sample_fallbacks() == 0
    for i, p in enumerate(prompts):
        assert sq.out[i] == replay(r, BIG_SEED, p, SP, BIG_STEPS), "sequence %d" % i
    m.close()
    r.close()
