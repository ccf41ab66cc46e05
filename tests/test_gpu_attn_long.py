"""The long-context prompt attention (attention_prompt_long.hip, contexts of 1025..2048 positions)
against the CPU oracle, bit for bit: the operator through lvk_attention_long, and whole evals on
n_ctx 2048 contexts, which lvk_prompt_attn_path must report on the new kernels.
"""
import os

import numpy as np
import pytest

from oracle_lib import gen_model, prompt_tokens

pytestmark = pytest.mark.gpu

TILE = 256      # the P.V position tile: PV_TILE of attention_prompt_long.hip
E, H = 512, 4


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lvk(gpu_available):
    import lvk as m
    return m


SMALL = [(0, 2, 256, 1), (29, 3, 256, 1), (31, 3, 256, 1), (60, 37, 256, 1), (10, 100, 256, 8), (0, 256, 256, 1),
         (TILE - 2, 3, 1024, 1), (2 * TILE - 2, 3, 1024, 1)]
# crosses 1024; an odd count of 8-token blocks (mirror pairing); the last positions; the window filled
LONG = [(1000, 70, 2048, 1), (900, 300, 2048, 4), (2046, 2, 2048, 1), (1800, 248, 2048, 1)]


@pytest.mark.parametrize("n_past,N,C,qs,qt,exp_path",
                         [c + (qt, ep) for c in SMALL for qt in (2, 3) for ep in ("computed", "table")] +
                         [c + (2, "computed") for c in LONG])
def test_attention_long(lvk, oracle, monkeypatch, n_past, N, C, qs, qt, exp_path):
    """f32 rows == orc_attention, blocks == the oracle's quantizer of those rows"""
    if exp_path == "table":
        monkeypatch.setenv("LVK_EXP_TABLE", "1")
    rng = np.random.default_rng(n_past * 17 + N + C)
    kc = rng.standard_normal(C * E).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(C * E).astype(np.float16).view(np.uint16).copy()
    q = (qs * rng.standard_normal(N * E)).astype(np.float32)
    want = np.zeros(N * E, np.float32)
    oracle.lib.orc_attention(kc, vc, q, E, H, C, n_past, N, want)
    got, blocks = lvk.attention_long(qt, kc, vc, q, E, H, C, n_past, N)
    want = want.reshape(N, E)
    bad = [t for t in range(N) if not np.array_equal(bits(got[t]), bits(want[t]))]
    assert not bad, "rows differ: %s" % bad[:8]
    bad = [t for t in range(N) if not np.array_equal(blocks[t], oracle.quantize(want[t], qt))]
    assert not bad, "blocks differ: %s" % bad[:8]


@pytest.mark.parametrize("qt,e,h,C,n_past,N", [(4, E, H, 256, 0, 2), (2, E, H, 2080, 0, 2), (2, E, H, 48, 0, 2),
                                               (2, 256, 4, 256, 0, 2), (2, E, H, 256, 0, 0), (2, E, H, 256, 255, 2)])
def test_attention_long_bad_arguments(lvk, qt, e, h, C, n_past, N):
    kc = np.zeros(C * e, np.uint16)
    with pytest.raises(RuntimeError):
        lvk.attention_long(qt, kc, kc, np.zeros(N * e, np.float32), e, h, C, n_past, N)


# 600 tokens at 0, 500 at 600, two single tokens; then 5 tokens (a batch below the 16 of the matmuls' tile)
STEPS = [(0, 600), (600, 500), (1100, 1), (1101, 1), (1102, 5)]
_want = {}


def _model(model_dir, ft):
    return gen_model(os.path.join(model_dir, "attn_long_w512_f%d.bin" % ft), n_embd=512, n_head=4, n_layer=2, ftype=ft)


def _oracle_logits(oracle, path):
    if path not in _want:
        om = oracle.model(path, 2048)
        toks = prompt_tokens(1107)
        _want[path] = [om.eval(toks[p:p + n], p).copy() for p, n in STEPS]
        om.close()
    return _want[path]


def _run(lvk, path, want_path):
    m = lvk.Llama(path, n_ctx=2048)
    try:
        assert m.prompt_attn_path(600) == want_path
        assert m.prompt_attn_path(1) == 3
        toks = prompt_tokens(1107)
        return [m.eval(toks[p:p + n], p).copy() for p, n in STEPS]
    finally:
        m.close()


@pytest.mark.parametrize("ft,long_on", [(2, True), (3, True), (1, True), (2, False)])
def test_model_n_ctx_2048(lvk, oracle, model_dir, monkeypatch, ft, long_on):
    """every logits row of prompt batches and decode steps on a 2048 context equals the oracle's, on the
    new kernels and (LVK_ATTN_LONG=0 before the context is made) on the generic route.  The f16 file
    (ft 1: the kernels' f32-rows output) is compared with the generic route instead: the CPU oracle
    reads Q4 matrices only (oracle/lvk_oracle.c mul_mat_q), and the reference build loads no 2-layer
    file; attention.hip's f32 rows are pinned to the oracle by test_gpu_ops.py::test_attention"""
    path = _model(model_dir, ft)
    if ft == 1:
        monkeypatch.setenv("LVK_ATTN_LONG", "0")
        want = _run(lvk, path, 0)
        monkeypatch.delenv("LVK_ATTN_LONG")
    else:
        want = _oracle_logits(oracle, path)
    if not long_on:
        monkeypatch.setenv("LVK_ATTN_LONG", "0")
    got = _run(lvk, path, 2 if long_on else 0)
    for (p, n), g, w in zip(STEPS, got, want):
        assert np.isfinite(g).all() and np.ptp(g) > 0
        assert np.array_equal(bits(g), bits(w)), "eval of %d tokens at %d" % (n, p)


def test_n_ctx_1024_keeps_its_kernels(lvk, model_dir):
    m = lvk.Llama(_model(model_dir, 2), n_ctx=1024)
    try:
        assert m.prompt_attn_path(600) == 1
    finally:
        m.close()
