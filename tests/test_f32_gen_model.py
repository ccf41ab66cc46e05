"""lvk-gen-model --ftype 0 is deterministic (no GPU): the generated tiny f32 file is the one
tests/golden/tiny_f32.npz was made from, byte for byte."""
import hashlib
import os
import struct
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
from make_golden_f32 import CFG, NAME  # noqa: E402


def test_tiny_f32_file_matches_golden_sha256(model_dir):
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
    assert hp["ftype"] == 0 and hp["n_layer"] == CFG["n_layer"] and hp["n_embd"] == CFG["n_embd"]


def test_tiny_f32_tensor_types_and_specials(model_dir):
    """every tensor is f32; the 2-D ones have exact zeros, -0 and f32 subnormals sprinkled in and
    carry full-precision mantissas (not f16 values widened)"""
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
        assert ft == 0
        size = 4 * ne[0] * (ne[1] if nd == 2 else 1)
        if nd == 2 and seen < 3:
            w = np.frombuffer(data, np.uint32, ne[0] * ne[1], d)
            assert (w == 0x00000000).any() and (w == 0x80000000).any()
            sub = ((w & 0x7f800000) == 0) & ((w & 0x7fffff) != 0)
            assert sub.any() and (w[sub] >> 31).any() and not (w[sub] >> 31).all()   # subnormals of both signs
            assert ((w & 0x7f800000) != 0x7f800000).all()                       # finite
            # the 13 mantissa bits an f16 lacks are in use: nearly no value is a widened f16
            # (one in 8192 has them all zero by chance), and they take thousands of patterns
            assert ((w & 0x1fff) != 0).mean() > 0.99 and len(np.unique(w & 0x1fff)) > 8000
            seen += 1
        off = d + size
    assert off == len(data) and seen == 3
