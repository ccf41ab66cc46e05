"""lvk_score_host (include/lvk_ops.h), no GPU: the host definition of the scoring tail equals a
restatement of the reference's softmax (examples/perplexity/perplexity.cpp:6-20) that calls this
host's libm expf per element -- bit for bit, special rows included -- and the scoring entry points
are exported.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "llama.vk_amd", "lib", "libllama_vk_amd.so")

_libm = C.CDLL("libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


@pytest.fixture(scope="module")
def lvk():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "llama.vk_amd"), "-j8"], stdout=subprocess.DEVNULL)
    import lvk as m
    return m


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ref_prob(row, target):
    """perplexity.cpp:6-20, then [target]: float max from logits[0] with std::max's rule, float
    subtraction, libm expf, double sum in index order, the float divided by the double sum"""
    row = np.asarray(row, np.float32)
    mx = row[0]
    for v in row:
        mx = v if mx < v else mx              # std::max(mx, v): the left operand unless mx < v
    s = 0.0
    e_t = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = row - mx                          # float32 - float32
    for i, di in enumerate(d):
        e = _libm.expf(float(di))
        s += e                                # double += float
        if i == target:
            e_t = np.float32(e)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(e_t) / np.float64(s))


def special_rows(V, rng):
    """(name, row, target) for the crafted rows of the scoring tests; V >= 5"""
    base = (rng.standard_normal(V) * 8).astype(np.float32)
    out = []
    r = base.copy()
    out.append(("target_is_argmax", r, int(np.argmax(r))))
    r = base.copy(); r[V - 1] = r.max() + 3
    out.append(("max_at_last", r, 1))
    r = base.copy(); r[1] = r[V - 2] = r.max() + 1
    out.append(("tied_max", r, V - 2))
    out.append(("all_equal", np.full(V, 1.25, np.float32), 3))
    r = (-30 + rng.standard_normal(V)).astype(np.float32); r[3] = 95
    out.append(("max_plus_95", r, 3))
    out.append(("max_plus_95_other", r.copy(), 0))
    r = np.zeros(V, np.float32); r[1] = 95
    out.append(("target_95_below", r, 0))
    r = np.zeros(V, np.float32); r[1] = 110
    out.append(("target_110_below", r, 0))
    r = base.copy(); r[0] = np.nan
    out.append(("nan_at_0", r, 2))
    r = base.copy(); r[V // 2] = np.nan
    out.append(("nan_in_middle", r, 1))
    r = base.copy(); r[V // 3] = np.inf
    out.append(("plus_inf", r, 0))
    out.append(("all_minus_inf", np.full(V, -np.inf, np.float32), 1))
    return out


def assert_same_float(a, b, what):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(b):
        assert np.isnan(a), what
    else:
        assert bits(a) == bits(b), "%s: %r vs %r" % (what, a, b)


@pytest.mark.parametrize("V", [5, 32000])
def test_score_host_equals_reference_softmax(lvk, V):
    rng = np.random.default_rng(V)
    n = 6 if V == 5 else 1
    x = (rng.standard_normal((n, V)) * 8).astype(np.float32)
    t = rng.integers(0, V, n).astype(np.int32)
    got = lvk.score_host(x, t)
    for i in range(n):
        assert_same_float(got[i], ref_prob(x[i], int(t[i])), "row %d" % i)
        assert 0 < got[i] <= 1


@pytest.mark.parametrize("V", [5, 1000])
def test_score_host_special_rows(lvk, V):
    cases = special_rows(V, np.random.default_rng(3))
    x = np.stack([r for _, r, _ in cases])
    t = np.array([k for _, _, k in cases], np.int32)
    got = lvk.score_host(x, t)
    byname = {}
    for (name, row, k), g in zip(cases, got):
        assert_same_float(g, ref_prob(row, k), name)
        byname[name] = g
    assert bits(byname["target_110_below"]) == 0
    d = byname["target_95_below"]
    assert 0 < d < np.finfo(np.float32).tiny              # a denormal, not flushed
    assert np.isfinite(byname["max_plus_95"]) and byname["max_plus_95"] > 0.99
    for name in ("nan_at_0", "nan_in_middle", "plus_inf", "all_minus_inf"):
        assert np.isnan(byname[name]), name
    assert byname["all_equal"] == np.float32(1.0 / V)


def test_score_host_unscored_rows_and_refusals(lvk):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((3, 7)) * 8).astype(np.float32)
    got = lvk.score_host(x, [2, -1, 6])
    assert bits(got[1]) == bits(np.float32(-1.0))
    assert_same_float(got[0], ref_prob(x[0], 2), "row 0")
    assert_same_float(got[2], ref_prob(x[2], 6), "row 2")
    pr = np.zeros(3, np.float32)
    t = np.array([0, 7, 0], np.int32)                     # a target >= V
    assert lvk.lib.lvk_score_host(x, 3, 7, t, pr.ctypes.data) == -1
    assert lvk.lib.lvk_score_host(x, 3, 7, np.zeros(3, np.int32), None) == -1
    assert lvk.lib.lvk_score_host(x, 0, 7, np.zeros(3, np.int32), pr.ctypes.data) == -1


def test_scoring_symbols_exported(lvk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for s in ("lvk_score_rows", "lvk_score_host", "lvk_eval_score", "lvk_decode_batch_score"):
        assert s in exported, s
    from test_abi import declared_symbols
    assert not [s for s in declared_symbols() if s not in exported]
    for f in ("score_rows", "score_host", "perplexity"):
        assert callable(getattr(lvk, f))
    assert callable(lvk.Llama.eval_score) and callable(lvk.Llama.decode_batch_score)
