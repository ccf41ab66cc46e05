"""Single-token decode of a Q4_1 model with the LLaMA 30B (6656 / 17920) or 65B (8192 / 22016) row lengths
on matvec_cu41_long.hip (lvk_decode_cu_active): a prompt and 8 teacher-forced steps bit-identical to the
CPU oracle, the captured chains (lvk_decode_chain, lvk_decode_greedy) equal to the per-step evals, and
LVK_DECODE_LONG=0 back on the generic kernels with the same logits bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, STEPS = 256, 8
PROMPT = [1, 450, 4996, 17354, 1701, 29916]
# name: (n_embd, n_head, n_layer, seed)
SHAPES = {"30b": (6656, 52, 1, 17), "65b": (8192, 64, 1, 19)}


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode_vs_oracle_chains_and_switch(lvk, oracle, model_dir, shape):
    from oracle_lib import forced_tokens, gen_model
    e, h, l, s = SHAPES[shape]
    path = gen_model(os.path.join(model_dir, "w%d_l%d_q41.bin" % (e, l)), n_embd=e, n_head=h, n_layer=l, ftype=3, seed=s)
    seq = [int(t) for t in forced_tokens(STEPS, seed=43)]
    m = lvk.Llama(path, n_ctx=N_CTX)
    assert m.decode_cu_active() == 1
    om = oracle.model(path, N_CTX)
    toks = np.array(PROMPT, np.int32)
    assert np.array_equal(bits(m.eval(toks, 0)), bits(om.eval(toks, 0)))
    am, dg = [], []
    for i, tok in enumerate(seq):
        a = m.eval([tok], len(PROMPT) + i)
        assert np.array_equal(bits(a), bits(om.eval([tok], len(PROMPT) + i))), "n_past %d" % (len(PROMPT) + i)
        am.append(int(np.argmax(a[-1])))
        dg.append(lvk.logits_digest(a[-1]))
    om.close()
    # the captured graphs over the same positions: teacher-forced, then greedy behind the first token
    got, gdg = m.decode_chain(seq, len(PROMPT))
    assert got.tolist() == am and gdg.tolist() == dg
    greedy, _ = m.decode_chain(seq[:1], len(PROMPT), STEPS)
    assert greedy[0] == am[0] and m.decode_greedy(seq[0], len(PROMPT), STEPS).tolist() == greedy.tolist()
    m.close()
    # the generic route in a process of its own
    code = ("import sys; sys.path.insert(0, %r); import lvk; m = lvk.Llama(%r, n_ctx=%d); m.eval(%r, 0); "
            "print('active', m.decode_cu_active(), [lvk.logits_digest(m.eval([t], %d + i)[-1]) for i, t in enumerate(%r)]); "
            "m.close()" % (os.path.join(ROOT, "llama.vk_amd"), path, N_CTX, PROMPT, len(PROMPT), seq))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LVK_DECODE_LONG="0"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "active 0 %s" % [int(d) for d in dg] in r.stdout, r.stdout + r.stderr
