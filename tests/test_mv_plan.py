"""CPU: the plan of the whole-corpus MaxSim scan (super-rag_amd/csrc/sr_mv_plan.h) under AddressSanitizer
+ UBSan.

The header is plain host C++ (no HIP call or header), so tests/native/mv_plan_test.cpp is built as a
program of its own with -fsanitize=address,undefined and run.  It checks that slabs tile [0, n_rows)
without gap or overlap for slab_rows 1, 7, n_rows - 1, n_rows, n_rows + 1 and the default, that the
token windows tile each slab at row boundaries and the spans each window, the span rule on rows of 0
tokens at either end, a row longer than the target, an all-empty slab and n_rows == 0 (the offsets
arrays hold exactly n_rows + 1 entries, so a read past them is a sanitizer report), Q >= 1 and the LDS
bytes within 160 KiB minus the static state for every dim, and the default slab_rows at B = 1, 32 and
1024.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("SR_HOST_CXX", "/opt/rocm/llvm/bin/clang++")


@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of ROCm not available")
def test_mv_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mv_plan_test")
    b = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "super-rag_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "mv_plan_test.cpp"), "-o", exe],
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
