"""CPU: the staging carver (super-rag_amd/csrc/sr_carve.h) under AddressSanitizer + UBSan.

The header is host-only, so tests/native/carve_test.cpp is built as plain C++ (no device code, no
HIP headers) with -fsanitize=address,undefined and run as a program of its own.  It declares the
layouts of every host entry point at B = 1, k = 1, dim = 3 and at B = 3, k = 5, dim = 20, layouts
with zero-count parts and single-part layouts over a host buffer of exactly bytes() bytes, and
checks that every part starts on a 256-byte multiple, that parts neither overlap nor leave bytes(),
and that writing every element of every part through its typed pointer raises no sanitizer report.
No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("SR_HOST_CXX", "/opt/rocm/llvm/bin/clang++")


@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of ROCm not available")
def test_carver_layouts_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "carve_test")
    b = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "super-rag_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "carve_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    print(out[-2000:])
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in r.stdout
