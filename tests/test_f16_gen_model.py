"""lvk-gen-model --ftype 1 is deterministic (no GPU): the generated tiny f16 file is the one
tests/golden/tiny_f16.npz was made from, byte for byte."""
import hashlib
import os
import struct
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden_f16 import CFG, NAME  # noqa: E402


def test_tiny_f16_file_matches_golden_sha256(model_dir):
    from oracle_lib import gen_model
    import lvk
    path = gen_model(os.path.join(model_dir, NAME + ".bin"), **CFG)
    g = np.load(os.path.join(GOLD, NAME + ".npz"), allow_pickle=False)
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 20), b""):
            h.update(b)
    assert h.hexdigest() == str(g["model_sha256"])
    hp = lvk.model_hparams(path)
    assert hp["ftype"] == 1 and hp["n_layer"] == CFG["n_layer"] and hp["n_embd"] == CFG["n_embd"]


def test_tiny_f16_tensor_types_and_specials(model_dir):
    """2-D tensors are f16 with exact zeros, -0 and subnormals sprinkled in; 1-D tensors f32"""
    from oracle_lib import gen_model
    path = gen_model(os.path.join(model_dir, NAME + ".bin"), **CFG)
    data = open(path, "rb").read()
    off = 36
    for _ in range(struct.unpack_from("<I", data, 8)[0]):
        off += 4 + struct.unpack_from("<I", data, off)[0] + 4
    seen = 0
    while off < len(data):
        nd, nl, ft = struct.unpack_from("<III", data, off)
        ne = struct.unpack_from("<%dI" % nd, data, off + 12)
        d = off + 12 + 4 * nd + nl
        d += (32 - d % 32) % 32
        assert ft == (1 if nd == 2 else 0)
        size = (2 if nd == 2 else 4) * ne[0] * (ne[1] if nd == 2 else 1)
        if nd == 2 and seen < 3:
            w = np.frombuffer(data, np.uint16, ne[0] * ne[1], d)
            assert (w == 0x0000).any() and (w == 0x8000).any()
            assert (((w & 0x7c00) == 0) & ((w & 0x3ff) != 0)).any()             # subnormals
            assert ((w & 0x7c00) != 0x7c00).all()                               # finite
            assert len(np.unique(w & 0x3ff)) == 1024                            # full 10-bit mantissas
            seen += 1
        off = d + size
    assert off == len(data) and seen == 3
