"""Dev tool: aggregate decode rate of a batched decode step (lvk_decode_batch), one row per
sequence, against the single-sequence llama_eval decode of the same process.
usage: seq_batch_speed.py [7b|13b|7b-f16 ...] [--steps N] [--out FILE]
Synthetic models (the bench's seeded files under /tmp/lvk_bench), n_ctx 512.  Slot 0 is filled by
a 511-token prompt and copied to slots 1..64 at lengths spread evenly over 16..511; a step
evaluates one row at the end of each of the first S slots, S = 1, 2, 4, ..., 64 (7b) or 16 (the
others), and is repeated at the same positions (a rewind).  Per S: the median step time over
`steps` steps after 3 warm-up steps, with the logits rows copied out and with only the device
argmax; aggregate tok/s = S / step time.  The yardstick is llama_eval (the captured decode graph)
on slot 0 at the 64 positions.  The per-class device profile is taken at S = 16.  Appends one
record per model to the JSON file (default profiles/seq_batch_speed.json) and prints it.
--chain [--repeats R] [--parent FILE ...]: the chained leg instead (run_chain): lvk_decode_batch_chain
against the host-fed legs, every leg R times, into profiles/seq_chain_speed.json; FILEs are records
this tool wrote at the parent commit.
--sample [--repeats R]: the sampled leg instead (run_sample): lvk_decode_batch_sample against the
argmax-only and the logits-to-host steps at 1, 16 and 64 sequences, into profiles/seq_sample_speed.json."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'llama.vk_amd'))
import numpy as np
import lvk

CFG = {'7b': ('llama-7b-q4_0.bin', dict(n_embd=4096, n_head=32, n_layer=32, ftype=2, seed=1)),
       '13b': ('llama-13b-q4_1.bin', dict(n_embd=5120, n_head=40, n_layer=40, ftype=3, seed=2)),
       '7b-f16': ('llama-7b-f16.bin', dict(n_embd=4096, n_head=32, n_layer=32, ftype=1, seed=1))}
N_CTX = 512
N_SLOT = 64


def spread(n):
    """n positions spread evenly over 16..511 (the middle one for n = 1)"""
    if n == 1:
        return [(16 + N_CTX - 1) // 2]
    return [16 + (i * (N_CTX - 1 - 16)) // (n - 1) for i in range(n)]


def median_ms(fn, steps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def run(name, steps):
    fn, cfg = CFG[name]
    path = os.path.join('/tmp/lvk_bench', fn)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
    sweep = [1, 2, 4, 8, 16, 32, 64] if name == '7b' else [16]
    m = lvk.Llama(path, n_ctx=N_CTX)
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX - 1)], np.int32)
    m.eval(toks, 0)
    m.seq_init(1 + max(sweep))
    row_tok = [int(100 + (s * 104729) % 31000) for s in range(N_SLOT)]

    # the yardstick: single-sequence llama_eval on slot 0 at the 64 positions
    pos64 = spread(N_SLOT)
    for p in pos64[:8]:
        m.eval([row_tok[0]], p)
    ts = []
    for i, p in enumerate(pos64):
        t0 = time.perf_counter()
        m.eval([row_tok[i]], p)
        ts.append(time.perf_counter() - t0)
    single = {'positions': len(pos64), 'tok_s': round(len(ts) / sum(ts), 1), 'median_ms': round(float(np.median(ts)) * 1e3, 3)}
    m.eval(toks, 0)          # slot 0 holds the prompt again

    rec = {'model': name + ' synthetic', 'n_ctx': N_CTX, 'steps': steps, 'weight_bytes': m.weight_bytes(),
           'single_sequence_llama_eval': single, 'batch': []}
    for S in sweep:
        pos = spread(S)
        for s, p in enumerate(pos):
            m.seq_copy(1 + s, 0, p)
        seqs = [1 + s for s in range(S)]
        ms = median_ms(lambda: m.decode_batch(row_tok[:S], seqs, pos), steps)
        ms_am = median_ms(lambda: m.decode_batch(row_tok[:S], seqs, pos, logits=False, argmax=True), steps)
        line = {'S': S, 'step_ms': round(ms, 3), 'tok_s': round(S / ms * 1e3, 1),
                'vs_single': round(S / ms * 1e3 / single['tok_s'], 2),
                'argmax_only_step_ms': round(ms_am, 3), 'argmax_only_tok_s': round(S / ms_am * 1e3, 1)}
        if S == 16:
            m.set_profiling(True)
            m.reset_profile()
            for _ in range(4):
                m.decode_batch(row_tok[:S], seqs, pos)
            p1 = m.profile()
            m.set_profiling(False)
            line['kernels_us_per_launch'] = {k: round(v['ms'] / v['launches'] * 1e3, 2) for k, v in p1.items() if v['launches']}
            line['class_ms_per_step'] = {k: round(v['ms'] / 4, 3) for k, v in p1.items() if v['launches']}
        rec['batch'].append(line)
        print(json.dumps(line), flush=True)
    if len(sweep) > 1:       # the whole sweep only: a single S says nothing about smaller ones
        beat = [b['S'] for b in rec['batch'] if b['tok_s'] > single['tok_s']]
        rec['smallest_S_beating_single'] = min(beat) if beat else None
    m.close()
    return rec


def spread_pct(v):
    """run-to-run spread of repeated medians: (max - min) / median, in percent"""
    return round((max(v) - min(v)) / float(np.median(v)) * 100, 2)


def run_chain(name, steps, repeats, parents):
    """the chained leg (--chain): per S, `steps` steps of S rows in one lvk_decode_batch_chain call
    (3 warm-up steps in a call of their own, which also builds the step graph for S rows), per-step
    time = call time / steps, against the host-fed lvk_decode_batch legs of run() measured in this
    process: same slots, same window filling, the chain starting at min(position, n_ctx - steps) and
    moving on from there where the host-fed legs rewind.  Two further legs: the chain with the graph
    off (the same launches enqueued eagerly), and the host-fed argmax-only loop timed as the chain
    is (the whole of `steps` steps / steps).  Every leg is repeated `repeats` times;
    the figures are medians over the repeats, the spread is (max - min) / median.  parents: records
    written by this tool at the parent commit (their host-fed legs, one file per repeat)."""
    fn, cfg = CFG[name]
    path = os.path.join('/tmp/lvk_bench', fn)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
    sweep = [1, 2, 4, 8, 16, 32, 64] if name == '7b' else [16]
    m = lvk.Llama(path, n_ctx=N_CTX)
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX - 1)], np.int32)
    m.eval(toks, 0)
    m.seq_init(1 + max(sweep))
    row_tok = [int(100 + (s * 104729) % 31000) for s in range(N_SLOT)]
    pos64 = spread(N_SLOT)
    for p in pos64[:8]:
        m.eval([row_tok[0]], p)
    ts = []
    for i, p in enumerate(pos64):
        t0 = time.perf_counter()
        m.eval([row_tok[i]], p)
        ts.append(time.perf_counter() - t0)
    single = {'positions': len(pos64), 'tok_s': round(len(ts) / sum(ts), 1), 'median_ms': round(float(np.median(ts)) * 1e3, 3)}
    m.eval(toks, 0)
    model = name + ' synthetic'
    prec = [[r for r in json.load(open(f)) if r['model'] == model] for f in parents]
    prec = [r[0] for r in prec if r]
    rec = {'model': model, 'n_ctx': N_CTX, 'steps': steps, 'repeats': repeats, 'weight_bytes': m.weight_bytes(),
           'single_sequence_llama_eval': single, 'parent_commit_repeats': len(prec), 'chain': []}
    for S in sweep:
        pos = spread(S)
        for s, p in enumerate(pos):
            m.seq_copy(1 + s, 0, p)
        seqs = [1 + s for s in range(S)]
        cpos = [min(p, N_CTX - steps) for p in pos]
        host, host_am, chain, eager, loop = [], [], [], [], []

        def loop_ms():
            # the host-fed loop timed as the chain is: the whole of `steps` argmax-only steps / steps
            for _ in range(3):
                m.decode_batch(row_tok[:S], seqs, pos, logits=False, argmax=True)
            t0 = time.perf_counter()
            for _ in range(steps):
                m.decode_batch(row_tok[:S], seqs, pos, logits=False, argmax=True)
            return (time.perf_counter() - t0) / steps * 1e3

        def chain_ms():
            m.decode_batch_chain(row_tok[:S], seqs, cpos, 3)
            t0 = time.perf_counter()
            m.decode_batch_chain(row_tok[:S], seqs, cpos, steps)
            return (time.perf_counter() - t0) / steps * 1e3

        for _ in range(repeats):
            host.append(median_ms(lambda: m.decode_batch(row_tok[:S], seqs, pos), steps))
            host_am.append(median_ms(lambda: m.decode_batch(row_tok[:S], seqs, pos, logits=False, argmax=True), steps))
            loop.append(loop_ms())
            chain.append(chain_ms())
            m.set_graph(0)          # the same launches enqueued eagerly
            eager.append(chain_ms())
            m.set_graph(1)
        h, ha, c = float(np.median(host)), float(np.median(host_am)), float(np.median(chain))
        line = {'S': S, 'host_fed_step_ms': round(h, 3), 'host_fed_argmax_only_step_ms': round(ha, 3),
                'host_fed_spread_pct': spread_pct(host), 'host_fed_argmax_only_spread_pct': spread_pct(host_am),
                'chain_step_ms': round(c, 3), 'chain_spread_pct': spread_pct(chain), 'chain_tok_s': round(S / c * 1e3, 1),
                'chain_vs_host_fed_argmax_only': round(ha / c, 3), 'chain_vs_host_fed': round(h / c, 3),
                'chain_vs_single': round(S / c * 1e3 / single['tok_s'], 2),
                'chain_graph_off_step_ms': round(float(np.median(eager)), 3), 'chain_graph_off_spread_pct': spread_pct(eager),
                'host_fed_loop_step_ms': round(float(np.median(loop)), 3), 'host_fed_loop_spread_pct': spread_pct(loop),
                'chain_vs_host_fed_loop': round(float(np.median(loop)) / c, 3)}
        pl = [[b for b in r['batch'] if b['S'] == S] for r in prec]
        pl = [b[0] for b in pl if b]
        if pl:
            ph, pa = [b['step_ms'] for b in pl], [b['argmax_only_step_ms'] for b in pl]
            line['parent_host_fed_step_ms'] = round(float(np.median(ph)), 3)
            line['parent_host_fed_argmax_only_step_ms'] = round(float(np.median(pa)), 3)
            line['parent_host_fed_spread_pct'] = spread_pct(ph)
            line['parent_host_fed_argmax_only_spread_pct'] = spread_pct(pa)
            line['chain_vs_parent_host_fed_argmax_only'] = round(float(np.median(pa)) / c, 3)
        rec['chain'].append(line)
        print(json.dumps(line), flush=True)
    m.close()
    return rec


def run_sample(name, steps, repeats):
    """the sampled leg (--sample): per S in 1, 16, 64, three legs over the same rows (run()'s slots and
    positions, rewound every step; the rows' tokens change from step to step, the same way in every
    leg, so the logits do), called through the C entry points with every argument built beforehand:
    (a) lvk_decode_batch with the device argmax only;
    (b) lvk_decode_batch_sample with top_k 40, top_p 0.95, temp 0.8, repeat_penalty 1.1 and a 64-token
        window per row;
    (c) lvk_decode_batch with the logits rows copied to the host and nothing done with them: a lower
        bound on what a sampler on the host costs a caller without (b).
    Each leg's figure is the median step over `steps` steps after 3 warm-up steps; the legs run one
    after the other `repeats` times; reported are the medians over the repeats, the run-to-run spread
    (max - min) / median, the differences (b) - (a) and (c) - (a) per repeat, and the rows of (b) that
    took the all-logits path."""
    fn, cfg = CFG[name]
    path = os.path.join('/tmp/lvk_bench', fn)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
    sweep = [1, 16, 64]
    m = lvk.Llama(path, n_ctx=N_CTX)
    toks = np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX - 1)], np.int32)
    m.eval(toks, 0)
    m.seq_init(1 + max(sweep))
    variants = 8
    row_tok = [np.array([100 + ((s + 64 * v) * 104729) % 31000 for s in range(N_SLOT)], np.int32) for v in range(variants)]
    wins = [np.ascontiguousarray(toks[7 * s:7 * s + 64]) for s in range(N_SLOT)]     # 64 ids per row, the rows' differ
    assert all(len(w) == 64 for w in wins)
    lib = lvk.lib
    rec = {'model': name + ' synthetic', 'n_ctx': N_CTX, 'steps': steps, 'repeats': repeats, 'weight_bytes': m.weight_bytes(),
           'sampler': {'top_k': 40, 'top_p': 0.95, 'temp': 0.8, 'repeat_penalty': 1.1, 'window': 64}, 'sample': []}
    for S in sweep:
        pos = np.array(spread(S), np.int32)
        for s, p in enumerate(pos):
            m.seq_copy(1 + s, 0, int(p))
        seqs = np.arange(1, S + 1, dtype=np.int32)
        rows = (lvk.lvk_row_sample * S)(*[lvk.lvk_row_sample(1, 40, 0.95, 0.8, 1.1, 64, wins[s].ctypes.data) for s in range(S)])
        out = np.zeros(S, np.int32)
        lg = np.zeros((S, m.n_vocab), np.float32)
        step = [0]

        def tok():
            step[0] += 1
            return np.ascontiguousarray(row_tok[step[0] % variants][:S])

        def leg_a():
            assert lib.lvk_decode_batch(m.ctx, tok(), seqs, pos, S, None, out.ctypes.data) == 0

        def leg_b():
            assert lib.lvk_decode_batch_sample(m.ctx, tok(), seqs, pos, S, ctypes.addressof(rows), out.ctypes.data) == 0

        def leg_c():
            assert lib.lvk_decode_batch(m.ctx, tok(), seqs, pos, S, lg.ctypes.data, None) == 0

        a, b, c = [], [], []
        f0 = m.sample_fallbacks()
        for _ in range(repeats):
            a.append(median_ms(leg_a, steps))
            b.append(median_ms(leg_b, steps))
            c.append(median_ms(leg_c, steps))
        ba, ca = [y - x for x, y in zip(a, b)], [y - x for x, y in zip(a, c)]
        line = {'S': S, 'argmax_only_step_ms': round(float(np.median(a)), 3), 'argmax_only_spread_pct': spread_pct(a),
                'sample_step_ms': round(float(np.median(b)), 3), 'sample_spread_pct': spread_pct(b),
                'logits_to_host_step_ms': round(float(np.median(c)), 3), 'logits_to_host_spread_pct': spread_pct(c),
                'sample_minus_argmax_ms': round(float(np.median(ba)), 3), 'sample_minus_argmax_ms_repeats': [round(v, 3) for v in ba],
                'logits_to_host_minus_argmax_ms': round(float(np.median(ca)), 3),
                'logits_to_host_minus_argmax_ms_repeats': [round(v, 3) for v in ca],
                'sample_tok_s': round(S / float(np.median(b)) * 1e3, 1),
                'sampled_rows': S * (steps + 3) * repeats, 'fallback_rows': m.sample_fallbacks() - f0}
        rec['sample'].append(line)
        print(json.dumps(line), flush=True)
    m.close()
    return rec


def main():
    args = sys.argv[1:]
    steps, out = 20, None
    names, chain, repeats, parents, sample = [], False, 3, [], False
    while args:
        a = args.pop(0)
        if a == '--steps':
            steps = int(args.pop(0))
        elif a == '--out':
            out = args.pop(0)
        elif a == '--chain':
            chain = True
        elif a == '--sample':
            sample = True
        elif a == '--repeats':
            repeats = int(args.pop(0))
        elif a == '--parent':
            parents.append(args.pop(0))
        else:
            names.append(a)
    out = out or os.path.join(ROOT, 'profiles', 'seq_sample_speed.json' if sample else
                              'seq_chain_speed.json' if chain else 'seq_batch_speed.json')
    recs = json.load(open(out)) if os.path.exists(out) else []
    for name in names or ['7b']:
        rec = (run_sample(name, steps, repeats) if sample else
               run_chain(name, steps, repeats, parents) if chain else run(name, steps))
        recs = [r for r in recs if r['model'] != rec['model']] + [rec]
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(recs, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
