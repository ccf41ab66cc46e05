"""bench.py's plain run and --dump-outputs on the GPU, on a tiny model (--model takes any ggjt
file that exists): the plain run prints the timed decode's fields and none of --full's legs, and
DIR/logits.npy is the logits row a caller of the timed path holds after its last step -- the
same bits from run to run, and the bits the same steps give in this process."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, N_CTX = 5, 2, 512
FULL_ONLY = ("roofline", "prompt_eval", "decode_greedy_device", "decode_13b_q4_1", "decode_65b_q4_0",
             "layer_split", "kernels", "cpu_baseline")


def _bench(model, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--model", model, "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "logits.npy"))


@pytest.fixture(scope="module")
def runs(tiny_models, tmp_path_factory, gpu_available):
    d = tmp_path_factory.mktemp("bench_dump")
    return [_bench(tiny_models["tiny_q4_0"], str(d / name)) for name in ("a", "b")]


def test_plain_line_has_the_timed_fields_only(runs):
    line = runs[0][0]
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "tok/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]


def test_dump_is_float32_logits_and_repeats_bit_for_bit(runs):
    (_, a), (_, b) = runs
    assert a.dtype == np.float32 and a.shape == (1, 32000) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_dump_is_the_last_timed_steps_logits(runs, tiny_models):
    """the bench's steps again in this process: prompt, the window filled greedily, the prompt
    again, then STEPS greedy steps at the bench's positions"""
    import lvk
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    m = lvk.Llama(tiny_models["tiny_q4_0"], n_ctx=N_CTX)
    tok = bench.fill_window(m, np.array(bench.prompt_tokens(16), np.int32), N_CTX)
    for i in range(STEPS):
        lg = m.eval([tok], bench.spread_pos(i, STEPS, N_CTX))
        tok = int(np.argmax(lg[-1]))
    m.close()
    assert np.array_equal(lg.view(np.uint32), runs[0][1].view(np.uint32))
