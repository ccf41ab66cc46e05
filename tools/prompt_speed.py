"""Dev tool: 7B 512-token prompt eval time (best of 3) and per-kernel-class milliseconds, plus
a hash of the last logits row (equal hashes across LVK_PROMPT_A16=0/1 = identical bits).
usage: prompt_speed.py [n_tokens] [7b|13b|65b] [n_ctx] [n_past]  (the bench's seeded files)
n_ctx (default 512) is the context's size; with n_past > 0 (default 0) the KV window below it is
filled by earlier evals of up to 512 tokens, and the timed batch starts there."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'llama.vk_amd'))
import numpy as np
import lvk

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
which = sys.argv[2] if len(sys.argv) > 2 else '7b'
fname, cfg = {'7b': ('llama-7b-q4_0.bin', dict(n_embd=4096, n_head=32, n_layer=32, ftype=2, seed=1)),
              '13b': ('llama-13b-q4_1.bin', dict(n_embd=5120, n_head=40, n_layer=40, ftype=3, seed=2)),
              '65b': ('llama-65b-q4_0.bin', dict(n_embd=8192, n_head=64, n_layer=80, ftype=2, seed=3))}[which]
path = '/tmp/lvk_bench/' + fname
if not os.path.exists(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
t0 = time.perf_counter()
n_ctx = int(sys.argv[3]) if len(sys.argv) > 3 else 512
n_past = int(sys.argv[4]) if len(sys.argv) > 4 else 0
m = lvk.Llama(path, n_ctx=n_ctx)
load_s = time.perf_counter() - t0
image = m.prompt_image_bytes()
toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, n_past + n)], np.int32)
for p0 in range(0, n_past, 512):
    m.eval(toks[p0:min(p0 + 512, n_past)], p0)
toks = toks[n_past:]
runs = []
for _ in range(3):
    t0 = time.perf_counter()
    lg = m.eval(toks, n_past)
    runs.append(time.perf_counter() - t0)
best = min(runs)
h = hashlib.sha1(np.ascontiguousarray(lg[-1]).tobytes()).hexdigest()[:16]
m.set_profiling(True)
m.reset_profile()
m.eval(toks, n_past)
p = m.profile()
attn_path = m.prompt_attn_path(n)
m.set_profiling(False)
m.close()
print(json.dumps({'model': which, 'a16': os.environ.get('LVK_PROMPT_A16', '1'), 'n': n, 'n_ctx': n_ctx, 'n_past': n_past,
                  'attn_path': attn_path, 'runs_ms': [round(r * 1e3, 2) for r in runs], 'ms': round(best * 1e3, 2),
                  'tok_s': round(n / best, 1), 'logits_sha1': h, 'a16_image_bytes': image, 'load_s': round(load_s, 2),
                  'kernels_ms': {k: round(v['ms'], 3) for k, v in p.items() if v['launches']}}), flush=True)
