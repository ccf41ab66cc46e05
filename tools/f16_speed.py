"""Dev tool: decode and prompt speed of the 7B-shaped f16 or f32 synthetic model (32 layers,
n_ctx 512, lvk-gen-model --ftype 1 | 0 --seed 1; a 13.5 GB / 27 GB file under /tmp/lvk_bench).
usage: f16_speed.py [steps] [ftype: 1 (default) f16, 0 f32]
Prints two JSON lines:
  decode: single-stream greedy decode with the window filled by a 512-token prompt, `steps`
          positions spread evenly over 16..511; tok/s, the step's fraction of the 8 TB/s
          roofline (weight bytes / step time), per-kernel microseconds and GB/s
  prompt: the 512-token prompt (best of 3), its fraction of the 157.3 TFLOP/s vector-fp32 peak
          at 2 flop per chain step, and the same 512 tokens fed one at a time through the
          decode kernels"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'llama.vk_amd'))
import numpy as np
import lvk

CFG = dict(n_embd=4096, n_head=32, n_layer=32, ftype=1, seed=1)
N_CTX = 512
PEAK_BW = 8.0e12
PEAK_FLOPS = 157.3e12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    ftype = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    if ftype not in (0, 1):
        sys.exit('ftype: 1 f16, 0 f32')
    name = '7b-f16' if ftype == 1 else '7b-f32'
    CFG['ftype'] = ftype
    path = '/tmp/lvk_bench/llama-%s.bin' % name
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **CFG)
    t0 = time.perf_counter()
    m = lvk.Llama(path, n_ctx=N_CTX)
    load_s = time.perf_counter() - t0
    wbytes = m.weight_bytes()
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX)], np.int32)

    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        lg = m.eval(toks, 0)
        best = min(best, time.perf_counter() - t0)
    m.set_profiling(True)
    m.reset_profile()
    m.eval(toks, 0)
    pp = m.profile()
    m.set_profiling(False)
    hp = lvk.model_hparams(path)
    E, L = hp['n_embd'], hp['n_layer']
    F = ((2 * (4 * E) // 3 + hp['n_mult'] - 1) // hp['n_mult']) * hp['n_mult']
    # chain steps: the layer matrices for every token, lm_head for the last one
    flop = 2.0 * (N_CTX * L * (4 * E * E + 3 * E * F) + hp['n_vocab'] * E)

    # decode: window filled by the prompt; positions spread evenly over 16..511
    pos = [16 + (i * (N_CTX - 16)) // steps for i in range(steps)]
    tok = int(np.argmax(lg[-1]))
    for p in pos[:8]:
        tok = int(np.argmax(m.eval([tok], p)[-1]))
    t0 = time.perf_counter()
    for p in pos:
        tok = int(np.argmax(m.eval([tok], p)[-1]))
    dt = (time.perf_counter() - t0) / steps
    m.set_profiling(True)
    m.reset_profile()
    for p in pos[::max(1, steps // 16)]:
        tok = int(np.argmax(m.eval([tok], p)[-1]))
    p1 = m.profile()
    m.set_profiling(False)
    ks = {k: round(v['ms'] / v['launches'] * 1e3, 2) for k, v in p1.items() if v['launches']}
    gbs = {k: round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 0) for k, v in p1.items() if v['launches'] and v.get('bytes')}
    print(json.dumps({'what': 'decode', 'model': name + ' synthetic', 'steps': steps, 'tok_s': round(1 / dt, 1),
                      'ms_per_token': round(dt * 1e3, 3), 'weight_bytes': wbytes,
                      'roofline_fraction': round(wbytes / dt / PEAK_BW, 3), 'kernels_us': ks, 'gbs': gbs,
                      'load_s': round(load_s, 1)}), flush=True)

    # the prompt's tokens one at a time through the decode kernels
    t0 = time.perf_counter()
    for i in range(N_CTX):
        m.eval([int(toks[i])], i)
    one_by_one = time.perf_counter() - t0
    m.close()
    print(json.dumps({'what': 'prompt', 'model': name + ' synthetic', 'n': N_CTX, 'ms': round(best * 1e3, 2),
                      'tok_s': round(N_CTX / best, 1), 'vector_fp32_fraction': round(flop / best / PEAK_FLOPS, 3),
                      'one_token_at_a_time_ms': round(one_by_one * 1e3, 1),
                      'kernels_ms': {k: round(v['ms'], 3) for k, v in pp.items() if v['launches']}}), flush=True)


if __name__ == '__main__':
    main()
