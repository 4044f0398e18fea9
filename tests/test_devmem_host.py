"""DevGroup, the owner of the engines' device buffers (csrc/devmem.h), on the CPU: tests/native/devmem_test.cpp defines the two
runtime functions the owner calls over malloc / free, with a "fail the k-th call" counter, and is built with AddressSanitizer
(leak detection included) and UBSan.  Failure paths of the engines' allocations cannot be reached on a GPU without exhausting
it; this is where they are covered."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


# a sanitizer build runs on development machines only
@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_devgroup_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "devmem_test")
    subprocess.check_call([CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "devmem_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "devmem ok" and r.stderr == "", r.stdout + r.stderr
