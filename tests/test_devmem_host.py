"""The owners of the engines' HIP resources on the CPU: the buffer groups (csrc/devmem.h), the decoder's step-graph cache and events
(csrc/hipres.h) and its per-row record tables (csrc/rowtable.h).  tests/native/*_test.cpp define the runtime functions an owner calls over malloc / free -- with a "fail the k-th
call" counter for the allocations -- and are built with AddressSanitizer (leak detection included) and UBSan.  Failure paths of the
engines' allocations cannot be reached on a GPU without exhausting it, and a graph cache is slow to fill there; this is where they
are covered.  The host plan of a generation (csrc/gen_plan.h) is built and run the same way: its refusals are plain arithmetic on
host records, which a GPU test could only reach one refused call at a time."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def run_sanitized(tmp_path, name):
    """Builds tests/native/<name>_test.cpp with AddressSanitizer and UBSan and runs it; its last word is '<name> ok'."""
    exe = str(tmp_path / f"{name}_test")
    subprocess.check_call([CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", f"{name}_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{name} ok" and r.stderr == "", r.stdout + r.stderr


# a sanitizer build runs on development machines only
@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_devgroup_under_asan_and_ubsan(tmp_path):
    run_sanitized(tmp_path, "devmem")   # DevGroup and PinnedGroup: the same checks on both


@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_stepgraphs_under_asan_and_ubsan(tmp_path):
    run_sanitized(tmp_path, "stepgraphs")   # StepGraphs and Event (csrc/hipres.h)


@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_rowtable_under_asan_and_ubsan(tmp_path):
    run_sanitized(tmp_path, "rowtable")   # RowTable (csrc/rowtable.h): failed allocations, set / copy_row / upload ranges, release


@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_gen_plan_under_asan_and_ubsan(tmp_path):
    run_sanitized(tmp_path, "gen_plan")   # plan_generation (csrc/gen_plan.h): kinds, flags, reserve and refusals of a tiny engine
