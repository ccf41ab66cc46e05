"""Dev tool: scoring one 511-token chunk of examples/perplexity (n_ctx 512: the 255 rows j >= 256
are scored) through the logits_all route and through lvk_eval_score.
usage: score_speed.py [--repeats R] [--out FILE]
The 7B Q4_0 synthetic model of seq_batch_speed.py (the bench's seeded file under /tmp/lvk_bench).
Legs, each the median of R (default 3) repeats after one warm-up:
(a) today's way: a logits_all context, llama_eval of the 511 tokens (all 511 logits rows to the
    host), then lvk_score_host over the 255 scored rows; the eval and the host softmax are also
    reported on their own;
(b) the new call: lvk_eval_score on a plain context with targets -1 for the first 256 rows;
(f) the forward pass alone: llama_eval of the 511 tokens on a plain context (last-token logits).
Also: the share of the 255 probabilities of (b) that are bit-equal to (a)'s and their largest
distance in ulp.  Writes one record to the JSON file (default profiles/score_speed.json) and
prints it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'llama.vk_amd'))
import numpy as np
import lvk

MODEL = ('llama-7b-q4_0.bin', dict(n_embd=4096, n_head=32, n_layer=32, ftype=2, seed=1))
N_CTX = 512


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def run(repeats):
    fn, cfg = MODEL
    path = os.path.join('/tmp/lvk_bench', fn)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
    n, half = N_CTX - 1, N_CTX // 2
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX)], np.int32)
    targets = np.full(n, -1, np.int32)
    targets[half:] = toks[half + 1:N_CTX]
    scored = np.ascontiguousarray(targets[half:])
    lib = lvk.lib

    a = lvk.Llama(path, n_ctx=N_CTX, logits_all=True)
    host = np.empty(n - half, np.float32)
    state = {}

    def a_eval():
        state['lg'] = a.eval(toks[:n], 0, copy=False)

    def a_score():
        rows = state['lg'][half:]
        assert lib.lvk_score_host(rows, n - half, a.n_vocab, scored, host.ctypes.data) == 0

    def leg_a():
        a_eval()
        a_score()

    ms_a, rep_a = timed(leg_a, repeats)
    ms_a_eval, _ = timed(a_eval, repeats)
    ms_a_score, _ = timed(a_score, repeats)
    want = host.copy()
    a.close()

    b = lvk.Llama(path, n_ctx=N_CTX)
    probs = np.empty(n, np.float32)
    tk = np.ascontiguousarray(toks[:n])

    def leg_b():
        assert lib.lvk_eval_score(b.ctx, tk, n, 0, targets.ctypes.data, probs.ctypes.data, None) == 0

    ms_b, rep_b = timed(leg_b, repeats)
    got = probs[half:].copy()
    ms_f, rep_f = timed(lambda: b.eval(tk, 0), repeats)
    b.close()

    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    dist = np.abs(ordered(got) - ordered(want))
    return {'model': '7b synthetic', 'n_ctx': N_CTX, 'tokens': n, 'scored_rows': int(n - half), 'repeats': repeats,
            'a_logits_all_eval_plus_host_softmax_ms': round(ms_a, 3), 'a_repeats_ms': rep_a,
            'a_eval_all_logits_to_host_ms': round(ms_a_eval, 3), 'a_host_softmax_ms': round(ms_a_score, 3),
            'b_eval_score_ms': round(ms_b, 3), 'b_repeats_ms': rep_b,
            'forward_pass_alone_ms': round(ms_f, 3), 'forward_repeats_ms': rep_f,
            'b_faster_than_a': bool(ms_b < ms_a), 'a_over_b': round(ms_a / ms_b, 3),
            'b_minus_forward_ms': round(ms_b - ms_f, 3),
            'bit_equal_share_pct': round(100.0 * float(np.mean(dist == 0)), 3), 'max_ulp': int(dist.max())}


def main():
    args = sys.argv[1:]
    repeats, out = 3, os.path.join(ROOT, 'profiles', 'score_speed.json')
    while args:
        k = args.pop(0)
        if k == '--repeats':
            repeats = int(args.pop(0))
        elif k == '--out':
            out = args.pop(0)
    rec = run(repeats)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump([rec], f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
