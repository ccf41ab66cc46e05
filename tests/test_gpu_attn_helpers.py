"""Score-helper workgroups of the decode attention (attention_decode.hip).

With n_head * 8 <= compute units (LLaMA-7B: 32 heads on 256 CUs) k_attn_d runs 4 score-only
helper workgroups per head beside the 4 slice workgroups, and in the exchange schedule
(n_kv > 128) the head's 64-position chunks are dealt over all 8: chunk c is scored by
workgroup c % 8.  The checked steps cross every edge of that deal at n_ctx 512 -- n_kv 128
(short schedule -> exchange), 192, 256 (the first helper chunk), 320, 448 and the full window
-- on a one-layer 7B-shaped Q4_0 file, teacher-forced (a seeded non-repeating token sequence;
the cache between two groups of steps is filled by prompt evals), bit for bit against the CPU
oracle, with the helpers on and with LVK_ATTN_HELPERS=0 (read once per process: child
processes), and with the step counter starting just below its 25-bit wrap (LVK_SEQ_START,
tests/test_gpu_seq_wrap.py) so that the tags the helpers publish wrap with everyone else's.
A 13B-shaped file (40 heads: 320 workgroups would not get a CU each) must keep the
4-workgroup launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import forced_tokens, gen_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX = 512
NKV_7B = (list(range(127, 132)) + list(range(191, 195)) + list(range(255, 259)) + list(range(319, 323)) +
          list(range(447, 451)) + [511, 512])
NKV_13B = list(range(127, 132)) + list(range(255, 259))


def _plan(nkvs):
    """[(n_past, n)]: single-token steps at n_kv = n_past + 1 in nkvs (n = 1), prompt evals between"""
    plan, pos = [], 0
    for n_kv in sorted(nkvs):
        p = n_kv - 1
        if p > pos:
            assert p - pos > 1           # a fill is a prompt eval, never a decode step
            plan.append((pos, p - pos))
        plan.append((p, 1))
        pos = p + 1
    return plan


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(pkg)r)
sys.path.insert(0, %(tests)r)
import lvk
from oracle_lib import forced_tokens
toks = forced_tokens(%(n_ctx)d)
m = lvk.Llama(%(model)r, n_ctx=%(n_ctx)d)
m.set_prompt_exact(True)
out = []
for n_past, n in %(plan)r:
    a = m.eval(toks[n_past:n_past + n], n_past)
    if n == 1:
        out.append(a[-1].copy())
np.savez(%(out)r, logits=np.stack(out), helpers=np.int32(lvk.attn_helpers_active(%(n_embd)d, %(n_head)d, %(n_ctx)d)))
m.close()
"""


def _run(model, out, nkvs, n_embd, n_head, env_extra):
    code = CHILD % {"pkg": os.path.join(ROOT, "llama.vk_amd"), "tests": os.path.join(ROOT, "tests"), "model": model,
                    "out": out, "plan": _plan(nkvs), "n_ctx": N_CTX, "n_embd": n_embd, "n_head": n_head}
    drop = ("LVK_ATTN_SHORT", "LVK_ATTN_NOEXCH", "LVK_ATTN_HELPERS", "LVK_SEQ_START")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def _oracle_logits(oracle, path, nkvs):
    om = oracle.model(path, N_CTX)
    toks, out = forced_tokens(N_CTX), []
    for n_past, n in _plan(nkvs):
        b = om.eval(toks[n_past:n_past + n], n_past)
        if n == 1:
            out.append(b[-1].copy())
    om.close()
    return np.stack(out)


@pytest.fixture(scope="module")
def model_7b(model_dir):
    return gen_model(os.path.join(model_dir, "w4096_l1_helpers.bin"), n_embd=4096, n_head=32, n_layer=1, ftype=2, seed=13)


@pytest.fixture(scope="module")
def want_7b(oracle, model_7b):
    w = _oracle_logits(oracle, model_7b, NKV_7B)
    w.setflags(write=False)
    return w


def _same(got, want, nkvs, what):
    assert got.shape == want.shape
    for i, n_kv in enumerate(sorted(nkvs)):
        assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), "%s: n_kv %d" % (what, n_kv)


def test_chunk_coverage_helpers_on_and_off(want_7b, model_7b, gpu_available, tmp_path):
    on = _run(model_7b, str(tmp_path / "on.npz"), NKV_7B, 4096, 32, {})
    off = _run(model_7b, str(tmp_path / "off.npz"), NKV_7B, 4096, 32, {"LVK_ATTN_HELPERS": "0"})
    assert int(on["helpers"]) == 4           # 32 * 8 workgroups on the MI355X's 256 CUs
    assert int(off["helpers"]) == 0
    _same(on["logits"], want_7b, NKV_7B, "helpers on")
    _same(off["logits"], want_7b, NKV_7B, "helpers off")
    _same(on["logits"], off["logits"], NKV_7B, "helpers on against off")


def test_epoch_wrap_with_helpers(want_7b, model_7b, gpu_available, tmp_path):
    # every eval takes one step-counter value: the counter wraps at the eval of n_kv 257, between
    # two steps whose chunk 4 is scored by a helper
    k = next(i for i, (n_past, n) in enumerate(_plan(NKV_7B)) if n == 1 and n_past + 1 == 257)
    got = _run(model_7b, str(tmp_path / "wrap.npz"), NKV_7B, 4096, 32, {"LVK_SEQ_START": str((1 << 25) - k)})
    _same(got["logits"], want_7b, NKV_7B, "step counter wrapping at n_kv 257")


def test_fallback_40_heads_keeps_four_workgroups(oracle, model_dir, gpu_available, tmp_path):
    path = gen_model(os.path.join(model_dir, "w5120_l1_helpers.bin"), n_embd=5120, n_head=40, n_layer=1, ftype=3, seed=14)
    got = _run(path, str(tmp_path / "fb.npz"), NKV_13B, 5120, 40, {})
    assert int(got["helpers"]) == 0          # 40 * 8 workgroups > 256 CUs
    _same(got["logits"], _oracle_logits(oracle, path, NKV_13B), NKV_13B, "40 heads")
