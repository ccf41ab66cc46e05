"""A batched decode step of a Q4_0 model with the 13B (5120 / 13824) or 65B (8192 / 22016) row lengths on
matvec_cols_long.hip (lvk_rows_cols_active): every logits row is bit-identical to the single-token
llama_eval at that position, the captured chain graph gives the digests of the same rows fed step by
step, and LVK_ROWS_COLS=0 turns the route off.  n = the n_ff tile + 1 takes a second launch of the W2
matmul (65B: 11); the 13B shape's measured limit is its tile, 16, so that is its larger n.  The 30B
pair is covered by tests/test_gpu_cols_long_ops.py alone.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, N_PRE, STEPS = 256, 140, 3
# name: (n_embd, n_head, n_layer, seed)
SHAPES = {"13b": (5120, 40, 2, 11), "65b": (8192, 64, 1, 12)}


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


@pytest.fixture(scope="module")
def models(model_dir):
    from oracle_lib import gen_model
    return {k: gen_model(os.path.join(model_dir, "w%d_l%d_q40.bin" % (e, l)), n_embd=e, n_head=h, n_layer=l, ftype=2, seed=s)
            for k, (e, h, l, s) in SHAPES.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape,n", [("13b", 2), ("13b", 16), ("65b", 2), ("65b", 11)])
def test_rows_match_single_token_evals(lvk, models, shape, n):
    from oracle_lib import forced_tokens
    model = models[shape]
    pre = forced_tokens(N_PRE, seed=31)
    lens = [20 + (i * (N_PRE - 20)) // (n - 1) for i in range(n)]      # the slots: one prefix at 20 .. 140
    slots = [1 + i for i in range(n)]
    tok, tok2 = forced_tokens(n, seed=32), forced_tokens(n, seed=33)
    # the reference rows, longest slot first: an eval at n_past = m reads only positions < m
    r = lvk.Llama(model, n_ctx=N_CTX)
    r.eval(pre, 0)
    want = {i: r.eval([int(tok[i])], lens[i])[-1].copy() for i in reversed(range(n))}
    r.close()

    def rows_context():
        c = lvk.Llama(model, n_ctx=N_CTX)
        c.seq_init(n + 1)
        c.eval(pre, 0)
        for i, k in enumerate(lens):
            c.seq_copy(1 + i, 0, k)
        return c

    m, h = rows_context(), rows_context()
    assert m.rows_cols_active(n) == 1
    lg, _ = m.decode_batch(tok, slots, lens)
    for i in range(n):
        assert np.array_equal(bits(lg[i]), bits(want[i])), "row %d of %d, n_past %d" % (i, n, lens[i])
    # the chained graph against the same rows fed step by step
    h.decode_batch(tok, slots, lens, logits=False, argmax=True)
    pos = [k + 1 for k in lens]
    got, dg, _ = m.decode_batch_chain(tok2, slots, pos, STEPS, digests=True)
    t = tok2
    for i in range(STEPS):
        row, am = h.decode_batch(t, slots, [p + i for p in pos], argmax=True)
        assert got[i].tolist() == am.tolist(), "tokens of step %d" % i
        assert dg[i].tolist() == [lvk.logits_digest(x) for x in row], "digests of step %d" % i
        t = am
    m.close()
    h.close()


def test_env_switch_turns_the_route_off(lvk, models):
    model = models["13b"]
    m = lvk.Llama(model, n_ctx=N_CTX)
    assert (m.rows_cols_active(2), m.rows_cols_active(16), m.rows_cols_active(17)) == (1, 1, 0)
    m.close()
    code = ("import sys; sys.path.insert(0, %r); import lvk; m = lvk.Llama(%r, n_ctx=%d); "
            "print('active', m.rows_cols_active(2), m.rows_cols_active(16)); m.close()"
            % (os.path.join(ROOT, "llama.vk_amd"), model, N_CTX))
    env = dict(os.environ, LVK_ROWS_COLS="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "active 0 0" in r.stdout, r.stdout + r.stderr
