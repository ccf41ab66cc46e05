"""Generate tests/golden/tiny_f32.npz from the REFERENCE build.

Run in the build container (needs oracle/_ref/libref.so, `make -C oracle ref`, and
llama.vk_amd/bin/lvk-gen-model).  The fixture is data only: the seeded tiny f32 model's
sha256 (it pins lvk-gen-model --ftype 0) and the reference's logits for make_golden.py's
chunking: prompt batches CHUNKS, then N_DECODE greedy single-token steps.

    python tests/golden/make_golden_f32.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import CHUNKS, N_DECODE, sha256  # noqa: E402
from make_golden_f16 import logits_from_planes  # noqa: E402,F401  (the tests take it from here)
from oracle_lib import Ref, gen_model, prompt_tokens  # noqa: E402

NAME = "tiny_f32"
# 32 layers: the reference loader aborts on a layer count other than 32 / 40 / 60 / 80
# (llama.cpp:741-749, llama_model_type_name)
CFG = dict(n_embd=256, n_head=2, n_layer=32, ftype=0, seed=7)


def main():
    ref = Ref()
    tmp = "/tmp/lvk_golden"
    os.makedirs(tmp, exist_ok=True)
    path = gen_model(os.path.join(tmp, NAME + ".bin"), **CFG)
    m = ref.model(path, 512)
    toks = prompt_tokens(sum(CHUNKS))
    steps, tokens_fed = [], []
    n_past = 0
    for ch in CHUNKS:
        lg = m.eval(toks[n_past:n_past + ch], n_past)
        steps.append(lg[-1])
        tokens_fed.append(toks[n_past:n_past + ch])
        n_past += ch
    tok = int(np.argmax(steps[-1]))
    for _ in range(N_DECODE):
        lg = m.eval([tok], n_past)
        steps.append(lg[-1])
        tokens_fed.append(np.array([tok], np.int32))
        n_past += 1
        tok = int(np.argmax(lg[-1]))
    m.close()
    # the logits as their four byte planes, as in make_golden_f16.py (the planes deflate below
    # the 1 MiB limit for committed files); tests rebuild them with logits_from_planes()
    planes = np.ascontiguousarray(np.stack(steps).astype("<f4").view(np.uint8).reshape(len(steps), -1, 4).transpose(2, 0, 1))
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), logits_planes=planes,
                        tokens=np.concatenate(tokens_fed), chunks=np.array([len(t) for t in tokens_fed], np.int32),
                        model_sha256=np.array(sha256(path)), cfg=np.array(json.dumps(CFG)))
    print("wrote %s.npz" % NAME)


if __name__ == "__main__":
    main()
