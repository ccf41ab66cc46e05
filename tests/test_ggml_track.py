"""The host change tracking behind ggml_graph_compute's device mirrors (llama.vk_amd/csrc/runtime/
ggml_track.cpp: which host pages must be uploaded again) on a CPU, without the library and without
a GPU: tools/ggml_graph/track_test.cpp is built from that one source file with AddressSanitizer and
UBSan linked in, and runs one case per process -- real mappings (private, read-only file, remapped,
mprotect'ed, shared, partly unmapped), the pinned-memory decision with a counting stand-in for
HIP's pointer query, the byte ranges of invalid pages against a brute-force restatement, the
validity carried into a merged mirror, and the span arithmetic -- under LVK_GGML_CACHE=1 and =2.
Under 2 the program reports whether the kernel's soft-dirty bits work: where they do, the
written / unwritten page checks run; where they do not, the tracker must fall back and every
case must behave as under 1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "ggml_graph", "bin", "track_test")
CASES = ["private", "ro-kept", "remap", "mprotect", "shared", "hole", "pinned", "edges", "adopt", "spans"]


@pytest.fixture(scope="module")
def track_test():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ggml_graph"), BIN], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("cache", ["1", "2"])
@pytest.mark.parametrize("case", CASES)
def test_tracking_case(track_test, case, cache):
    env = dict(os.environ, LVK_GGML_CACHE=cache, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([track_test, case], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and ("ok %s" % case) in r.stdout.splitlines(), (r.stdout[-2000:], r.stderr[-4000:])
    if cache == "2":
        first = r.stdout.splitlines()[0]
        assert first.startswith("soft-dirty: "), r.stdout
        print(case, first)
