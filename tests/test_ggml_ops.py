"""The per-operator cases of tools/ggml_graph/op_test.c without a GPU.

op_test.c runs one small graph per edge of every operator ggml_graph_compute dispatches (dup,
cpy, add, sub, mul, div, repeat, silu, scale, diag_mask_inf, rms_norm, soft_max, rope,
get_rows, mul_mat) and is built twice: on this library (tools/ggml_graph/bin/op_test_lvk) and
on the reference ggml.c (oracle/_ref/op_test_ref).  tests/test_gpu_ggml_ops.py compares the
two dumps bit for bit on the GPU; this file checks what can be checked on the CPU:

  * both builds construct the same result tensor for every case (op, type, shape, strides,
    whether it is a view of its source, pool accounting);
  * the reference's dump is what numpy computes from the dumped inputs for the element-wise
    operators, so the harness is not vacuous: inputs differ per case, outputs are written,
    and the dump order is the logical order;
  * the mul_mat and rms_norm inputs are such that the summation order shows in the bits.

Left out on purpose: a copy from an f16 source into another SHAPE.  The reference's dup_f16
wraps its destination counters at the source's extents (ggml.c:4871-4881, 4897-4907), which
leaves holes in or writes outside a destination of another shape; this library copies the
k-th element to the k-th element there (graph_ops.hip k_g_cpy), so there is nothing to
compare against.  Every f16-source case keeps the shape.
"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVK_BIN = os.path.join(ROOT, "tools", "ggml_graph", "bin", "op_test_lvk")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "op_test_ref")

Q4_0, Q4_1, I32, F16, F32 = 0, 1, 4, 5, 6
DTYPE = {I32: np.int32, F16: np.float16, F32: np.float32}
BLOCK_BYTES = {Q4_0: 20, Q4_1: 24}


def _build():
    if not os.path.exists(LVK_BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ggml_graph")], stdout=subprocess.DEVNULL)


def case_names():
    _build()
    return subprocess.run([LVK_BIN, "--list"], capture_output=True, text=True, check=True, timeout=60).stdout.split()


def build_only(binary):
    """{case: the line op_test prints for the case's result tensor}, nothing computed"""
    env = dict(os.environ, OP_TEST_BUILD_ONLY="1")
    if os.environ.get("LVK_LIB"):       # another build of the library (the sanitizer run)
        env["LD_LIBRARY_PATH"] = os.path.dirname(os.environ["LVK_LIB"])
    r = subprocess.run([binary], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


class Tensor:
    def __init__(self, type_, ne, raw):
        self.type, self.ne, self.raw = type_, ne, raw
        if type_ in DTYPE:
            self.a = np.frombuffer(raw, DTYPE[type_]).reshape(ne[::-1])     # [i3][i2][i1][i0]
        else:
            self.a = np.frombuffer(raw, np.uint8)

    def bits(self):
        return self.a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[self.a.itemsize])


def parse_dump(path):
    """{case: (inputs, outputs)} of an op_test dump, in file order"""
    buf = open(path, "rb").read()
    pos, out = 0, {}
    while pos < len(buf):
        (nl,) = struct.unpack_from("<I", buf, pos)
        name = buf[pos + 4:pos + 4 + nl].decode()
        pos += 4 + nl
        n_in, n_out = struct.unpack_from("<II", buf, pos)
        pos += 8
        ts = []
        for _ in range(n_in + n_out):
            (type_,) = struct.unpack_from("<i", buf, pos)
            ne = struct.unpack_from("<4q", buf, pos + 4)
            pos += 36
            n = ne[0] * ne[1] * ne[2] * ne[3]
            size = n // 32 * BLOCK_BYTES[type_] if type_ in BLOCK_BYTES else n * np.dtype(DTYPE[type_]).itemsize
            ts.append(Tensor(type_, ne, buf[pos:pos + size]))
            pos += size
        assert name not in out, name
        out[name] = (ts[:n_in], ts[n_in:])
    assert pos == len(buf)
    return out


def run_dump(binary, path, **kw):
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=120, **kw)
    assert r.returncode == 0, "%s exited %d: %s" % (os.path.basename(binary), r.returncode, r.stderr[-3000:])
    return parse_dump(path)


@pytest.fixture(scope="module")
def ref_dump(tmp_path_factory):
    _build()
    if not os.path.exists(REF_BIN):
        pytest.skip("reference build oracle/_ref/op_test_ref not present")
    return run_dump(REF_BIN, tmp_path_factory.mktemp("op_test") / "ref.bin")


def test_result_tensors_and_pool_match_reference():
    """topology: every case's result tensor -- op, type, ne, nb, whether its data is its
    source's (scale, cpy, diag_mask_inf, soft_max and rope return views in this reference
    version), ggml_used_mem -- is the same line for line in both builds"""
    _build()
    if not os.path.exists(REF_BIN):
        pytest.skip("reference build oracle/_ref/op_test_ref not present")
    a, b = build_only(REF_BIN), build_only(LVK_BIN)
    assert [ln.split(":")[0] for ln in a] == case_names()
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert not diff and len(a) == len(b), diff[:5]


def _same_bits(got, exp, what):
    """bit equality, except that a NaN only has to be a NaN"""
    assert got.a.shape == exp.shape and got.a.dtype == exp.dtype, what
    g, e = got.a.ravel(), np.ascontiguousarray(exp).ravel()
    differ = got.bits().ravel() != e.view(got.bits().dtype)
    if e.dtype.kind == "f":
        differ = np.where(np.isnan(e), ~np.isnan(g), differ)
    bad = np.flatnonzero(differ)
    assert bad.size == 0, "%s: %d elements differ, first %s: %r vs numpy %r" % (
        what, bad.size, bad[:5], g[bad[:5]], e[bad[:5]])


def _restate(name, ins, outs):
    """the expected first output in numpy, or None where the operator is not restated here"""
    op = name.split("_")[0]
    o = outs[0]
    with np.errstate(all="ignore"):
        if op in ("cpy", "dup"):
            return ins[0].a.ravel().astype(DTYPE[o.type]).reshape(o.a.shape)
        if op in ("add", "sub", "mul", "div"):
            f = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[op]
            return f(ins[0].a, ins[1].a)
        if op == "scale":
            return ins[0].a * ins[1].a.ravel()[0]
        if op == "repeat":
            s = ins[0].a
            return np.tile(s, [o.a.shape[k] // s.shape[k] for k in range(4)])
        if op == "diag":
            x = ins[0].a.copy()
            n_past = int(ins[1].a.ravel()[0])
            i0 = np.arange(x.shape[3])[None, None, None, :]
            i1 = np.arange(x.shape[2])[None, None, :, None]
            x[np.broadcast_to(i0 > n_past + i1, x.shape)] = -np.inf
            return x
        if op == "get" and ins[0].type in (F16, F32):
            return ins[0].a[0, 0][ins[1].a.ravel()].astype(np.float32)[None, None]
        if op == "rms":
            # ggml.c:6060-6076: float squares summed in double in index order
            x = ins[0].a
            s = np.zeros(x.shape[:3], np.float64)
            for k in range(x.shape[3]):
                s += (x[..., k] * x[..., k]).astype(np.float64)
            mean = (s / x.shape[3]).astype(np.float32)
            scale = np.float32(1.0) / np.sqrt(mean + np.float32(1e-6))
            return x * scale[..., None]
    return None


def test_reference_dump_is_what_numpy_computes(ref_dump):
    """cpy / dup (np.float16 rounds to nearest even), add, sub, mul, div, scale, repeat,
    diag_mask_inf, get_rows of f16 / f32 and rms_norm restated from the dumped inputs equal
    the reference's dumped output bit for bit; so do the bytes a strided destination leaves
    alone and the elements rope must not touch"""
    assert list(ref_dump) == case_names()
    restated = set()
    for name, (ins, outs) in ref_dump.items():
        exp = _restate(name, ins, outs)
        if exp is not None:
            _same_bits(outs[0], exp, name)
            restated.add(name.split("_")[0])
    assert restated == {"cpy", "dup", "add", "sub", "mul", "div", "scale", "repeat", "diag", "get", "rms"}

    # a copy into 3 columns of rows 16 apart from element 5 changes those 24 elements only
    for name in ("cpy_f32_f16_into_vcache", "cpy_f16_f16_into_vcache"):
        ins, outs = ref_dump[name]
        exp = ins[1].a.copy().ravel()
        src = ins[0].a[0, 0].astype(np.float16)                # [i1][i0]: 8 rows of 3
        for i1 in range(8):
            exp[5 + 16 * i1:5 + 16 * i1 + 3] = src[i1]
        _same_bits(outs[1], exp.reshape(outs[1].a.shape), name + " (cache)")
        assert (outs[1].bits() != ins[1].bits()).sum() >= 20, name

    # rope: dims from n_dims on, and in mode 1 the slices below n_past, keep their bits
    for name, (ins, outs) in ref_dump.items():
        if not name.startswith("rope_") or name == "rope_m0_view":
            continue
        x, y = ins[0], outs[0]
        n_past, n_dims, mode = (int(v) for v in ins[1].a.ravel())
        keep = np.zeros(x.a.shape, bool)
        keep[..., n_dims:] = True
        if mode != 0:
            keep[:, :n_past] = True
        assert np.array_equal(y.bits()[keep], x.bits()[keep]), name
        if not keep.all():
            changed = (y.bits() != x.bits()) & ~keep
            assert changed.sum() > (~keep).sum() // 2, name     # p = 0 slices rotate by nothing
    ins, outs = ref_dump["rope_m0_view"]
    w0, w1 = ins[0], outs[1]
    assert np.array_equal(w1.bits()[..., [0, 9]], w0.bits()[..., [0, 9]])
    assert np.array_equal(w1.bits()[..., 1:9], outs[0].bits())
    assert not np.array_equal(w1.bits()[..., 1:9], w0.bits()[..., 1:9])

    # the generator is seeded per case: no two random cases share their first input
    rnd = [n for n in ref_dump if not n.endswith("_special") and n != "silu_sweep"]
    firsts = {bytes(ref_dump[n][0][0].raw) for n in rnd}
    assert len(firsts) == len(rnd)
    # every output was written: it is not the zero fill of a new tensor
    for name, (ins, outs) in ref_dump.items():
        assert any(outs[0].raw), name


def _mm_cases(dump):
    for name, (ins, outs) in dump.items():
        m = re.match(r"mm_(f16|f32)_", name)
        if m and ins[0].ne[0] >= 33:
            yield name, m.group(1), ins, outs


def test_mul_mat_inputs_depend_on_summation_order(ref_dump):
    """every f16 / f32 mul_mat case with K >= 33 has at least one output element whose
    reference bits (4 x 8 FMA lanes over K & ~31, the reduce tree, then the tail) differ
    from a plain left-to-right float32 sum of the same products: a kernel that sums in
    another order cannot pass these cases.  A condition on the inputs (seed, magnitudes,
    per-case salt in op_test.c), checked here on the CPU."""
    n = 0
    for name, kind, ins, outs in _mm_cases(ref_dump):
        x = ins[0].a.astype(np.float32)                       # [i3][i2][M][K]
        y = ins[1].a
        if kind == "f16":
            y = y.astype(np.float16).astype(np.float32)       # the INIT phase, ggml.c:6412-6428
        acc = np.zeros(outs[0].a.shape, np.float32)           # [i3][i2][N][M]
        big = np.zeros(outs[0].a.shape, np.float32)
        for k in range(x.shape[3]):
            p = y[:, :, :, None, k] * x[:, :, None, :, k]
            acc = acc + p
            big = np.maximum(big, np.abs(p))
        # the same operation: each of the K additions of either order rounds a partial sum of at
        # most K * max|product| by at most 2^-24 of it
        K = x.shape[3]
        assert np.all(np.abs(acc - outs[0].a) <= big * (2 * K * K * 2.0 ** -24)), name
        differ = int((acc.view(np.uint32) != outs[0].bits()).sum())
        print("%s: plain sum differs in %d of %d elements" % (name, differ, acc.size))
        assert differ >= 1, name
        n += 1
    assert n == 2 * (4 * 4 + 3)


def test_rms_norm_inputs_depend_on_double_sum(ref_dump):
    """the mixed-magnitude rms_norm rows (terms near 1e4 among terms near 1e-3) come out with
    other bits when the squares are summed in float32 instead of double (ggml.c:6060-6063)"""
    ins, outs = ref_dump["rms_norm_mixed_magnitude"]
    x = ins[0].a
    s = np.zeros(x.shape[:3], np.float32)
    for k in range(x.shape[3]):
        s = s + x[..., k] * x[..., k]
    mean = s / np.float32(x.shape[3])
    y = x * (np.float32(1.0) / np.sqrt(mean + np.float32(1e-6)))[..., None]
    assert y.dtype == np.float32
    assert np.allclose(y, outs[0].a, rtol=1e-5, atol=0)
    rows = (y.view(np.uint32) != outs[0].bits()).any(axis=3)
    print("float sum changes %d of %d rows" % (rows.sum(), rows.size))
    assert rows.all()
