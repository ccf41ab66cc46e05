"""Scoring on the device (lvk_score_rows / lvk_eval_score / lvk_decode_batch_score, include/lvk_ops.h).

The definition is lvk_score_host, the reference's softmax(row)[target] (perplexity.cpp:6-20) with
this host's expf, pinned bit for bit in tests/test_score_host.py.  The device rounds a
double-precision exp where the host calls expf (both within 1 ulp of the true value, so e_target
may be the adjacent float) and the quotient is rounded once more: every finite result is within
2 ulp of the host twin, counted on the floats' ordered integer representations (denormals
included); 0, NaN and -1.0f match exactly.  The bound is derived, not measured.  Every test prints
the share of compared positions that are bit-equal.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from make_golden_f16 import CFG as CFG_F16, NAME as NAME_F16  # noqa: E402
from make_golden_f32 import CFG as CFG_F32, NAME as NAME_F32  # noqa: E402
from test_score_host import special_rows  # noqa: E402

ULP = 2
TALLY = {"equal": 0, "total": 0}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ordered(a):
    """floats -> integers in the same order, adjacent floats 1 apart (+0 and -0 both 0)"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def check_probs(dev, host, what):
    """the accuracy contract of the module docstring, element by element"""
    dev, host = np.asarray(dev, np.float32).reshape(-1), np.asarray(host, np.float32).reshape(-1)
    assert dev.shape == host.shape, what
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(dev), nan), "%s: NaN positions differ" % what
    exact = ~nan & ((host == 0) | (host == -1))
    assert np.array_equal(bits(dev[exact]), bits(host[exact])), "%s: a 0 / -1.0f result differs" % what
    fin = ~nan & ~exact
    dist = np.abs(ordered(dev[fin]) - ordered(host[fin]))
    eq = int(np.sum(dist == 0))
    TALLY["equal"] += eq
    TALLY["total"] += int(fin.sum())
    print("%s: %d finite positions, %d bit-equal (%.3f %%), max distance %d ulp; running share %.3f %% of %d"
          % (what, fin.sum(), eq, 100.0 * eq / max(1, fin.sum()), dist.max() if dist.size else 0,
             100.0 * TALLY["equal"] / max(1, TALLY["total"]), TALLY["total"]))
    assert dist.size == 0 or dist.max() <= ULP, "%s: %d ulp at position %d" % (what, dist.max(), np.flatnonzero(fin)[dist.argmax()])


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


# ---------------------------------------------------------------- op level
@pytest.mark.parametrize("V,n", [(1, 3), (5, 4), (1000, 3), (32000, 1), (32000, 3), (32000, 130), (32001, 3)])
def test_score_rows_random(lvk, V, n):
    """8 * standard_normal rows; V = 32001 and V = 5 put every row but the first off the 16-byte
    boundary (head and tail singles), V = 1 has no 16-byte load at all; n = 130 is more workgroups
    than one pass over an XCD's units"""
    rng = np.random.default_rng(1000 * V + n)
    x = (rng.standard_normal((n, V)) * 8).astype(np.float32)
    t = rng.integers(0, V, n).astype(np.int32)
    dev, am = lvk.score_rows(x, t, argmax=True)
    check_probs(dev, lvk.score_host(x, t), "V=%d n=%d" % (V, n))
    assert np.array_equal(am, np.argmax(x, axis=1))
    assert np.array_equal(bits(lvk.score_rows(x, t)), bits(dev))          # without the argmax: the same


@pytest.mark.parametrize("V", [5, 1000, 32000, 32001])
def test_score_rows_crafted(lvk, V):
    cases = special_rows(V, np.random.default_rng(V + 1))
    x = np.stack([r for _, r, _ in cases])
    t = np.array([k for _, _, k in cases], np.int32)
    dev, am = lvk.score_rows(x, t, argmax=True)
    host = lvk.score_host(x, t)
    check_probs(dev, host, "crafted V=%d" % V)
    by = {name: (d, a, row) for (name, row, _), d, a in zip(cases, dev, am)}
    assert by["target_is_argmax"][0] > 0 and by["max_at_last"][1] == V - 1
    assert bits(by["target_110_below"][0]) == 0
    assert 0 < by["target_95_below"][0] < np.finfo(np.float32).tiny       # denormal, not flushed
    assert np.isfinite(by["max_plus_95"][0]) and by["max_plus_95"][0] > 0.99
    assert bits(by["max_plus_95_other"][0]) == 0
    for name in ("nan_at_0", "nan_in_middle", "plus_inf", "all_minus_inf"):
        assert np.isnan(by[name][0]), name
    assert by["all_equal"][0] == np.float32(1.0 / V)
    for name, (_, a, row) in by.items():
        if not np.isnan(row).any():
            assert a == int(np.argmax(row)), name                         # first maximum (tied_max: the lower index)


def test_score_rows_unscored_row_between_scored(lvk):
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((3, 32000)) * 8).astype(np.float32)
    t = np.array([17, -1, 31999], np.int32)
    dev, am = lvk.score_rows(x, t, argmax=True)
    host = lvk.score_host(x, t)
    assert bits(dev[1]) == bits(np.float32(-1.0))
    check_probs(dev, host, "unscored between scored")
    alone = np.concatenate([lvk.score_rows(x[0], [17]), lvk.score_rows(x[2], [31999])])
    assert np.array_equal(bits(alone), bits(dev[[0, 2]]))                  # the neighbours do not notice
    assert np.array_equal(am, np.argmax(x, axis=1))                        # the argmax covers unscored rows too


def test_score_rows_refusals(lvk):
    x = np.zeros((2, 8), np.float32)
    pr = np.zeros(2, np.float32)
    L = lvk.lib
    assert L.lvk_score_rows(x, 2, 8, np.array([0, 8], np.int32), pr.ctypes.data, None) == -1
    assert L.lvk_score_rows(x, 2, 8, np.array([0, 1], np.int32), None, None) == -1
    big = np.zeros((1, 32769), np.float32)                                 # past the kernel's registers
    assert L.lvk_score_rows(big, 1, 32769, np.zeros(1, np.int32), pr.ctypes.data, None) == -1
    assert L.lvk_score_host(big, 1, 32769, np.zeros(1, np.int32), pr.ctypes.data) == 0


# ---------------------------------------------------------------- prompt path
def prompt_case(lvk, path, f16_kv, what):
    from oracle_lib import forced_tokens
    n_ctx, n = 128, 127
    toks = forced_tokens(n_ctx + 1, seed=31)
    targets = toks[1:n + 1].astype(np.int32).copy()
    targets[:64] = -1
    a = lvk.Llama(path, n_ctx=n_ctx, logits_all=True, f16_kv=f16_kv)
    lg_a = a.eval(toks[:n], 0)
    host = lvk.score_host(lg_a, targets)
    a.close()
    b = lvk.Llama(path, n_ctx=n_ctx, f16_kv=f16_kv)
    dev, am = b.eval_score(toks[:n], 0, targets, argmax=True)
    assert np.array_equal(bits(dev[:64]), bits(np.full(64, -1.0, np.float32)))
    assert np.all(dev[64:] > 0)
    check_probs(dev, host, what + " prompt")
    assert b.seq_tokens(0) == n and b.kv_cache_token_count() == n
    # the cache is llama_eval's: the next token's logits equal a context that took eval()
    t = int(toks[n])
    assert np.array_equal(am, np.argmax(lg_a, axis=1))
    c = lvk.Llama(path, n_ctx=n_ctx, f16_kv=f16_kv)
    c.eval(toks[:n], 0)
    row_b, row_c = b.eval([t], n), c.eval([t], n)
    assert np.array_equal(bits(row_b), bits(row_c)), what
    # one token: the matvec lm_head
    tgt = int(toks[n + 1])
    one, am1 = b.eval_score([t], n, [tgt], argmax=True)
    check_probs(one, lvk.score_host(row_c, [tgt]), what + " single token")
    assert int(am1[0]) == int(np.argmax(row_c[0]))
    assert b.seq_tokens(0) == n + 1
    b.close()
    c.close()


@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_q4_1", "tiny_f16", "tiny_f32"])
def test_eval_score_prompt_path(lvk, models, name):
    prompt_case(lvk, models[name], True, name)


def test_eval_score_prompt_path_f32_kv(lvk, models):
    prompt_case(lvk, models["tiny_q4_0"], False, "tiny_q4_0 f16_kv=False")


def test_eval_score_short_batches_and_logits_all_context(lvk, models):
    """15 tokens (below the matrix-core tile: the per-row kernels) at n_past > 0, on a logits_all
    context, whose host logits the call leaves alone"""
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    toks = forced_tokens(40, seed=32)
    a = lvk.Llama(path, n_ctx=64, logits_all=True)
    a.eval(toks[:20], 0)
    want = a.eval(toks[20:35], 20)
    targets = toks[21:36].astype(np.int32)
    host = lvk.score_host(want, targets)
    b = lvk.Llama(path, n_ctx=64, logits_all=True)
    b.eval(toks[:20], 0)
    check_probs(b.eval_score(toks[20:35], 20, targets), host, "15 tokens at n_past 20")
    assert b.seq_tokens(0) == 35
    a.close()
    b.close()


def test_host_route_is_the_host_twin(lvk, models, monkeypatch):
    """a vocabulary the kernel does not take is scored by lvk_score_host over the rows in HBM;
    LVK_SCORE_HOST=1 (read when a context is created) sends this 32000-entry model that way:
    every result bit-equal to the host twin, prompt and rows path, unscored rows and argmax too"""
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    toks = forced_tokens(41, seed=34)
    targets = toks[1:41].astype(np.int32).copy()
    targets[:7] = -1
    a = lvk.Llama(path, n_ctx=128, logits_all=True)
    lg = a.eval(toks[:40], 0)
    a.close()
    host = lvk.score_host(lg, targets)
    monkeypatch.setenv("LVK_SCORE_HOST", "1")
    b = lvk.Llama(path, n_ctx=128)
    monkeypatch.delenv("LVK_SCORE_HOST")
    dev, am = b.eval_score(toks[:40], 0, targets, argmax=True)
    assert np.array_equal(bits(dev), bits(host))
    assert np.array_equal(am, np.argmax(lg, axis=1))
    r = lvk.Llama(path, n_ctx=128)
    r.eval(toks[:40], 0)
    row, _ = r.decode_batch([int(toks[40])], [0], [40])
    got = b.decode_batch_score([int(toks[40])], [0], [40], [5])
    assert np.array_equal(bits(got), bits(lvk.score_host(row, [5])))
    b.close()
    r.close()


# ---------------------------------------------------------------- rows path
@pytest.mark.parametrize("name", ["tiny_q4_0", "tiny_f16"])
def test_decode_batch_score_rows(lvk, models, name):
    """the four-slot setup of test_gpu_seq_batch.test_rows_match_single_token_evals (offsets 0, 29,
    61, 125 at n_ctx 256), 2 steps: probs against the host twin on the rows decode_batch returns
    for an identically prepared context"""
    from oracle_lib import forced_tokens
    path = models[name]
    n_ctx, steps = 256, 2
    offs, slots = [29, 61, 125, 0], [1, 2, 0, 3]
    toks = [forced_tokens(offs[s] + steps + 1, seed=11 + s) for s in range(4)]

    def prepared():
        m = lvk.Llama(path, n_ctx=n_ctx)
        m.seq_init(4)
        for s in range(4):
            if offs[s]:
                m.eval(toks[s][:offs[s]], 0)
                if slots[s] != 0:
                    m.seq_copy(slots[s], 0, offs[s])
        return m
    m, r = prepared(), prepared()
    for k in range(steps):
        tok = [int(toks[s][offs[s] + k]) for s in range(4)]
        pos = [offs[s] + k for s in range(4)]
        tgt = np.array([int(toks[s][offs[s] + k + 1]) for s in range(4)], np.int32)
        if k == 1:
            tgt[2] = -1
        lg, am_want = r.decode_batch(tok, slots, pos, argmax=True)
        dev, am = m.decode_batch_score(tok, slots, pos, tgt, argmax=True)
        check_probs(dev, lvk.score_host(lg, tgt), "%s rows step %d" % (name, k))
        assert np.array_equal(am, am_want)
        assert [m.seq_tokens(s) for s in range(4)] == [r.seq_tokens(s) for s in range(4)]
        assert [m.seq_tokens(slots[s]) for s in range(4)] == [offs[s] + k + 1 for s in range(4)]
    m.close()
    r.close()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_unchanged(lvk, models):
    from oracle_lib import forced_tokens
    path = models["tiny_q4_0"]
    n_ctx = 128
    toks = forced_tokens(40, seed=33)
    m, fresh = lvk.Llama(path, n_ctx=n_ctx), lvk.Llama(path, n_ctx=n_ctx)
    m.eval(toks[:8], 0)
    fresh.eval(toks[:8], 0)
    L = lvk.lib
    t = np.ascontiguousarray(toks[8:28], np.int32)
    good = np.ascontiguousarray(toks[9:29], np.int32)
    pr = np.zeros(20, np.float32)
    bad = good.copy()
    bad[7] = m.n_vocab
    assert L.lvk_eval_score(m.ctx, t, 20, 8, bad.ctypes.data, pr.ctypes.data, None) == -1        # a target >= n_vocab
    assert L.lvk_eval_score(m.ctx, t, 20, 8, good.ctypes.data, None, None) == -1                 # null probs
    assert L.lvk_eval_score(m.ctx, t, 20, n_ctx - 19, good.ctypes.data, pr.ctypes.data, None) == -1   # n_past + n > n_ctx
    assert L.lvk_eval_score(m.ctx, t, 20, 8, None, pr.ctypes.data, None) == -1                   # null targets
    seqs, pos = np.zeros(20, np.int32), np.arange(8, 28, dtype=np.int32)
    assert L.lvk_decode_batch_score(m.ctx, t, seqs, pos, 20, bad.ctypes.data, pr.ctypes.data, None) == -1
    assert L.lvk_decode_batch_score(m.ctx, t, seqs, pos, 20, good.ctypes.data, None, None) == -1
    assert L.lvk_decode_batch_score(m.ctx, t, seqs, pos + 1, 20, good.ctypes.data, pr.ctypes.data, None) == -1   # a hole
    assert m.seq_tokens(0) == 8
    assert np.array_equal(bits(m.logits()), bits(fresh.logits()))           # llama_get_logits still the prompt's
    assert np.array_equal(bits(m.eval(toks[8:28], 8)), bits(fresh.eval(toks[8:28], 8)))
    assert np.array_equal(bits(m.eval([int(toks[28])], 28)), bits(fresh.eval([int(toks[28])], 28)))
    m.close()
    fresh.close()


def test_stage_context_is_refused(lvk, models):
    m = lvk.Llama(models["tiny_q4_0"], n_ctx=128, layers=(0, 16))
    pr = np.zeros(2, np.float32)
    t = np.array([5, 6], np.int32)
    assert lvk.lib.lvk_eval_score(m.ctx, t, 2, 0, t.ctypes.data, pr.ctypes.data, None) == -1
    m.close()


# ---------------------------------------------------------------- end to end
def test_perplexity_matches_reference_program(lvk, tiny_models, tmp_path):
    """lvk.perplexity over the text and arguments of test_dropin's perplexity test against the
    `[i]ppl,` fields the reference build of examples/perplexity prints.  Tolerance per printed
    value b: half a unit of its fourth decimal plus the 2-ulp bound carried through -log and the
    mean, |a - b| <= 0.5e-4 + 2.4e-7 * b (2 * 2^-23 = 2.4e-7)."""
    ref_exe = os.path.join(ROOT, "oracle", "_ref", "perplexity")
    if not os.path.exists(ref_exe):
        pytest.skip("%s not built (make -C oracle needs the reference sources)" % ref_exe)
    words = ["the", "model", "reads", "every", "token", "of", "this", "text", "and", "predicts", "next",
             "one", "from", "its", "context", "window", "while", "perplexity", "measures", "surprise"]
    text = " ".join(words[(i * 7) % len(words)] + ("." if i % 11 == 10 else "") for i in range(600))
    f = tmp_path / "ppl.txt"
    f.write_text(text)
    p = subprocess.run([ref_exe, "-m", tiny_models["tiny_q4_0"], "-f", str(f), "-c", "128", "-s", "1", "-t", "8"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    want = [float(b) for _, b in re.findall(rb"\[(\d+)\]([0-9.]+),", p.stdout)]
    assert len(want) >= 3
    m = lvk.Llama(tiny_models["tiny_q4_0"], n_ctx=128)
    got = lvk.perplexity(m, m.tokenize(text, add_bos=True), 128)
    m.close()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        print("chunk %d: %.7f vs the reference's %.4f" % (i + 1, a, b))
        assert abs(a - b) <= 0.5e-4 + 2.4e-7 * b, "chunk %d: %r vs %r" % (i + 1, a, b)
