"""Every ggml graph operator on the GPU against the reference ggml.c, case by case.

tools/ggml_graph/op_test.c (one small graph per operator edge: dup, cpy, add, sub, mul, div,
repeat, silu, scale, diag_mask_inf, rms_norm, soft_max, rope, get_rows, mul_mat of f16 / f32 /
Q4_0 / Q4_1) runs once on this library (every node on the GPU) and once on the reference's CPU
AVX2 build; each case's record must agree: same tensor types and shapes, byte-identical
inputs, bit-identical output in every element.  The one exemption: where the reference's
element is a NaN, the GPU's must be a NaN at the same index, sign and payload free (an x86
0/0 is a negative quiet NaN, and nothing in this project consumes NaN bits).

Left out on purpose: a copy from an f16 source into another shape.  The reference's dup_f16
wraps its destination counters at the source's extents (ggml.c:4871-4881, 4897-4907) and
leaves holes or writes outside the destination; k_g_cpy copies the k-th element to the k-th
element there, and no case compares the two.
"""
import os
import re

import numpy as np
import pytest

from test_ggml_ops import LVK_BIN, REF_BIN, ROOT, build_only, case_names, run_dump

pytestmark = pytest.mark.gpu

CASES = case_names()


@pytest.fixture(scope="module")
def dumps(gpu_available, tmp_path_factory):
    """both programs run every case once; the tests below only compare bytes"""
    if not os.path.exists(REF_BIN):
        pytest.skip("reference build oracle/_ref/op_test_ref not present")
    d = tmp_path_factory.mktemp("op_test")
    return run_dump(REF_BIN, d / "ref.bin"), run_dump(LVK_BIN, d / "lvk.bin")


@pytest.mark.parametrize("case", CASES)
def test_operator_case_matches_reference_ggml(dumps, case):
    ref, lvk = dumps
    assert case in ref and case in lvk
    (rin, rout), (gin, gout) = ref[case], lvk[case]
    assert len(rin) == len(gin) and len(rout) == len(gout) and len(rout) >= 1
    for i, (a, b) in enumerate(zip(rin + rout, gin + gout)):
        assert (a.type, a.ne) == (b.type, b.ne), "%s: tensor %d is %s %s here, %s %s in the reference" % (
            case, i, b.type, b.ne, a.type, a.ne)
    for i, (a, b) in enumerate(zip(rin, gin)):
        assert a.raw == b.raw, "%s: input %d differs between the two builds" % (case, i)
    for i, (a, b) in enumerate(zip(rout, gout)):
        differ = a.bits().ravel() != b.bits().ravel()
        if a.a.dtype.kind == "f":
            differ = np.where(np.isnan(a.a.ravel()), ~np.isnan(b.a.ravel()), differ)
        bad = np.flatnonzero(differ)
        assert bad.size == 0, "%s: output %d differs in %d of %d elements, first %s: reference %r (%s), GPU %r (%s)" % (
            case, i, bad.size, differ.size, bad[:5].tolist(), a.a.ravel()[bad[:5]].tolist(),
            ["%x" % v for v in a.bits().ravel()[bad[:5]]], b.a.ravel()[bad[:5]].tolist(),
            ["%x" % v for v in b.bits().ravel()[bad[:5]]])


def test_cases_cover_every_dispatched_operator():
    """every operator run_node dispatches to a kernel is the result of at least one case, so
    an operator added to ggml_graph_compute cannot ship without a case"""
    src = open(os.path.join(ROOT, "llama.vk_amd", "csrc", "runtime", "ggml_graph.cpp")).read()
    body = src[src.index("void run_node("):src.index("bool writes_data(")]
    dispatched = set(re.findall(r"case (GGML_OP_\w+):", body))
    dispatched -= {"GGML_OP_NONE", "GGML_OP_RESHAPE", "GGML_OP_VIEW", "GGML_OP_PERMUTE", "GGML_OP_TRANSPOSE"}
    assert len(dispatched) >= 15
    hdr = open(os.path.join(ROOT, "include", "ggml.h")).read()
    enum = re.search(r"enum ggml_op \{(.*?)\};", hdr, re.S).group(1)
    value = {n: i for i, n in enumerate(re.findall(r"(GGML_OP_\w+)", enum))}
    assert value["GGML_OP_NONE"] == 0
    built = {int(re.search(r": op (\d+) ", ln).group(1)) for ln in build_only(LVK_BIN)}
    missing = sorted(n for n in dispatched if value[n] not in built)
    assert not missing, "no op_test case for %s" % missing
