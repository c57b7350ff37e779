"""AddressSanitizer + UndefinedBehaviorSanitizer run of the Inception-v3 executor's HOST side (tests/test_sanitize_host.py does the same for the other handles).

inception.cpp and api.cpp are compiled from the real sources with ``-fsanitize=address,undefined -fno-gpu-sanitize`` (hipcc ``--cuda-host-only``: no device
code, no GPU) and linked with tests/sanitize/stubs.cpp + incep_stubs.cpp (host malloc stands in for device memory; every launch stub touches the first and last
byte of each tensor the kernel would access).  tests/sanitize/incep_harness.cpp, a stand-alone program, drives create -> set_weight -> finalize -> preprocess ->
workspace_bytes -> forward with a workspace of exactly the requested size, the error paths, and a finalize with a weight missing.  Nothing is loaded
into Python under a sanitizer.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "consolver_amd", "csrc")
HOST_SOURCES = ["api.cpp", "inception.cpp"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_inception_host_under_asan_ubsan(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    flags = ["-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w", "-I" + os.path.join(ROOT, "include")]
    srcs = [os.path.join(CSRC, s) for s in HOST_SOURCES] + [os.path.join(ROOT, "tests", "sanitize", f) for f in ("stubs.cpp", "tune_default.cpp", "incep_stubs.cpp", "incep_harness.cpp")]
    objs, procs = [], []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        objs.append(o)
        procs.append((s, subprocess.Popen([hipcc] + flags + ["-c", s, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{s}:\n{out}"
    exe = str(tmp_path / "incep_harness")
    r = subprocess.run([hipcc, "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-o", exe] + objs, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-6000:]
    assert "incep sanitize harness: ok" in r.stdout
    assert "AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-6000:]
