"""Dev tool: single-sequence decode of the 13B- and 30B-shaped Q4_0 synthetic models on matvec_cu_long.hip
against the generic kernels (LVK_DECODE_LONG=0, the route of the parent commit), with the 65B shape
(k_mv_cu either way) as the control; with --wtype q4_1 the 30B- and 65B-shaped Q4_1 models on
matvec_cu41_long.hip against the same switch (profiles/decode_long41_speed.json).
usage: decode_long_speed.py [--wtype q4_0|q4_1] [--layers N] [--repeats R] [--shapes a,b,...] [--out FILE]
                            [--libs PARENT.so NEW.so]
One process per leg, the legs alternating, R repeats (default 3).  A leg: the model of
tools/seq_batch_speed.py cut to N layers (default 8; 0: the whole model), n_ctx 512, a 511-token prompt,
then llama_eval of one token at 64 positions spread over 16..511, three passes after a warm-up of 8
evals; the figure is the median eval (host clock around the call, which ends in the logits copy).  A
fourth pass with the profiling classes on gives the device time per role and token.  Per shape the record
holds the medians of the repeats, their spread (max - min) / median, and whether the new route beats the
old by more than twice the larger spread (the rule for routing a row length by default).
Writes profiles/decode_long_speed.json.
With --libs the two legs are two builds of the library (LVK_LIB) on the same route instead of the two
switch settings, for a refactor: per shape and per role the record holds each build's median device time
over the repeats with its spread, and whether the new build is slower than the parent's by more than
twice the larger of the two spreads (--out is then required)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'llama.vk_amd'))
import numpy as np
import lvk
from seq_batch_speed import CFG, N_CTX, spread, spread_pct


def model_path(name, layers, wtype='q4_0'):
    fn, cfg = CFG[name]
    if wtype == 'q4_1':         # the same shape and seed as a Q4_1 file
        fn, cfg = fn.replace('q4_0', 'q4_1'), dict(cfg, ftype=3)
    if layers:
        fn, cfg = fn.replace('.bin', '-l%d.bin' % layers), dict(cfg, n_layer=layers)
    path = os.path.join('/tmp/lvk_bench', fn)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        lvk.gen_model(path, vocab=os.path.join(ROOT, 'tests', 'golden', 'vocab32000.bin'), **cfg)
    return path


def leg(path):
    m = lvk.Llama(path, n_ctx=N_CTX)
    m.eval(np.array([1] + [100 + (i * 7919) % 31000 for i in range(1, N_CTX - 1)], np.int32), 0)
    pos = spread(64)
    tok = [int(100 + (s * 104729) % 31000) for s in range(64)]
    for p in pos[:8]:
        m.eval([tok[0]], p)
    ts = []
    for _ in range(3):
        for i, p in enumerate(pos):
            t0 = time.perf_counter()
            m.eval([tok[i]], p)
            ts.append(time.perf_counter() - t0)
    m.set_profiling(True)
    m.reset_profile()
    for i, p in enumerate(pos):
        m.eval([tok[i]], p)
    pr = m.profile()
    rec = {'decode_cu_active': m.decode_cu_active(), 'median_ms': round(float(np.median(ts)) * 1e3, 4),
           'tok_s': round(len(ts) / sum(ts), 1), 'weight_bytes': m.weight_bytes(),
           'class_us_per_token': {k: round(v['ms'] / len(pos) * 1e3, 2) for k, v in pr.items() if v['launches']}}
    m.close()
    print('LEG ' + json.dumps(rec), flush=True)


LIBS_WHAT = ('tools/decode_long_speed.py --libs PARENT NEW: two builds of the library on the same route, shapes cut to 8 layers, '
             'one process per leg, parent and new alternating, medians of the repeats; per role the device time per token; '
             'new_slower_by_rule: new - parent > twice the larger of the two spreads (max - min of the repeats)')


def libs_record(name, q41, layers, repeats, legs, med):
    """two builds on the same route: per role the medians of the repeats, their spreads, and the rule"""
    side = lambda w: {'decode_cu_active': legs[w][0]['decode_cu_active'], 'median_ms': round(float(np.median(med[w])), 4),
                      'repeats_ms': med[w], 'spread_ms': round(max(med[w]) - min(med[w]), 4)}
    roles = {}
    for k in legs['new'][0]['class_us_per_token']:
        v = {w: [x['class_us_per_token'][k] for x in legs[w]] for w in legs}
        m = {w: float(np.median(v[w])) for w in v}
        noise = max(max(x) - min(x) for x in v.values())
        roles[k] = {'parent_us': round(m['old'], 2), 'new_us': round(m['new'], 2), 'parent_repeats_us': v['old'],
                    'new_repeats_us': v['new'], 'new_minus_parent_us': round(m['new'] - m['old'], 2),
                    'twice_larger_spread_us': round(2 * noise, 2), 'new_slower_by_rule': bool(m['new'] - m['old'] > 2 * noise)}
    return {'model': '%s%s synthetic%s' % (name, ' q4_1' if q41 else '', ' %d layers' % layers if layers else ''),
            'n_ctx': N_CTX, 'repeats': repeats, 'weight_bytes': legs['new'][0]['weight_bytes'], 'parent': side('old'),
            'new': side('new'), 'roles_device_us_per_token': roles,
            'any_role_slower_by_rule': any(r['new_slower_by_rule'] for r in roles.values())}


def main():
    args = sys.argv[1:]
    layers, repeats, out, shapes, wtype, libs = 8, 3, None, None, 'q4_0', None
    while args:
        a = args.pop(0)
        if a == '--leg':
            return leg(args.pop(0))
        if a == '--layers':
            layers = int(args.pop(0))
        elif a == '--repeats':
            repeats = int(args.pop(0))
        elif a == '--shapes':
            shapes = args.pop(0).split(',')
        elif a == '--out':
            out = args.pop(0)
        elif a == '--wtype':
            wtype = args.pop(0)
        elif a == '--libs':
            libs = {'old': os.path.abspath(args.pop(0)), 'new': os.path.abspath(args.pop(0))}
    if wtype not in ('q4_0', 'q4_1'):
        sys.exit('--wtype: q4_0 or q4_1')
    if libs and not out:
        sys.exit('--libs needs --out')
    q41 = wtype == 'q4_1'
    out = out or os.path.join(ROOT, 'profiles', 'decode_long41_speed.json' if q41 else 'decode_long_speed.json')
    shapes = shapes or (['30b', '65b'] if q41 else ['13b-q4_0', '30b', '65b'])
    recs = json.load(open(out)) if os.path.exists(out) and not libs else []
    doc = json.load(open(out)) if os.path.exists(out) and libs else {'what': LIBS_WHAT, 'shapes': []}
    for name in shapes:
        path = model_path(name, layers, wtype)
        legs = {'new': [], 'old': []}
        for _ in range(repeats):
            for which in ('new', 'old'):
                env = dict(os.environ, LVK_DECODE_LONG='1' if which == 'new' or libs else '0')
                if libs:
                    env['LVK_LIB'] = libs[which]
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', path], env=env, capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit('leg %s of %s failed (%d): %s' % (which, name, r.returncode, r.stdout + r.stderr))
                legs[which].append(json.loads([l for l in r.stdout.splitlines() if l.startswith('LEG ')][-1][4:]))
                print(name, which, legs[which][-1]['median_ms'], flush=True)
        med = {w: [x['median_ms'] for x in legs[w]] for w in legs}
        if libs:
            rec = libs_record(name, q41, layers, repeats, legs, med)
            print(json.dumps(rec), flush=True)
            doc['shapes'] = [r for r in doc['shapes'] if r['model'] != rec['model']] + [rec]
            with open(out, 'w') as f:
                json.dump(doc, f, indent=1)
                f.write('\n')
            continue
        new, old = float(np.median(med['new'])), float(np.median(med['old']))
        noise = max((max(v) - min(v)) for v in med.values())
        mid = lambda w: sorted(legs[w], key=lambda x: x['median_ms'])[len(legs[w]) // 2]
        rec = {'model': '%s%s synthetic%s' % (name, ' q4_1' if q41 else '', ' %d layers' % layers if layers else ''), 'n_ctx': N_CTX, 'repeats': repeats,
               'weight_bytes': legs['new'][0]['weight_bytes'],
               'new': {'decode_cu_active': legs['new'][0]['decode_cu_active'], 'median_ms': round(new, 4), 'repeats_ms': med['new'],
                       'spread_pct': spread_pct(med['new']), 'class_us_per_token': mid('new')['class_us_per_token']},
               'old_LVK_DECODE_LONG_0': {'decode_cu_active': legs['old'][0]['decode_cu_active'], 'median_ms': round(old, 4),
                                         'repeats_ms': med['old'], 'spread_pct': spread_pct(med['old']),
                                         'class_us_per_token': mid('old')['class_us_per_token']},
               'old_over_new': round(old / new, 4), 'old_minus_new_ms': round(old - new, 4),
               'larger_spread_ms': round(noise, 4), 'twice_larger_spread_ms': round(2 * noise, 4), 'new_wins_by_rule': bool(old - new > 2 * noise)}
        print(json.dumps(rec), flush=True)
        recs = [r for r in recs if r['model'] != rec['model']] + [rec]
        with open(out, 'w') as f:
            json.dump(recs, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
