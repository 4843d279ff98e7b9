"""CPU: the GEMM launch planner (super-rag_amd/csrc/sr_gemm_plan.h) under AddressSanitizer + UBSan.

The header is plain host C++ (no HIP call or header), so tests/native/gemm_plan_test.cpp is built as a
program of its own with -fsanitize=address,undefined and run.  It checks the epilogue traits table row
by row, both profile-name tables, and the kernel family, persistence, grid, block, tile walk, split-K,
profile name and booked bytes that plan_gemm returns for the product shapes and for every threshold of
the rules (512 big tiles, the K-step floors, the statistics stride, the workspace size to the byte,
the fallbacks between families and the rejected requests), against literals read off the launchers
as they were before the header existed.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("SR_HOST_CXX", "/opt/rocm/llvm/bin/clang++")


@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of ROCm not available")
def test_gemm_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "gemm_plan_test")
    b = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "super-rag_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "gemm_plan_test.cpp"), "-o", exe],
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
