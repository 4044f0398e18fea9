"""The launch plan of the 16-bit GEMMs (csrc/gemm16_plan.h: plain C++, no HIP) on the CPU: tests/native/gemm16_plan_test.cpp holds the
table of calls and the plans they must get -- family, template parameters, geometry, tail word, refusals, for both dtypes and every
switch -- under AddressSanitizer and UBSan.  tests/test_gpu_gemm16_plan.py launches every family the plan can name."""
import pytest
import torch

from test_devmem_host import run_sanitized


# a sanitizer build runs on development machines only
@pytest.mark.skipif(torch.cuda.is_available(), reason="sanitizer run: CPU machines only")
def test_gemm16_plan_under_asan_and_ubsan(tmp_path):
    run_sanitized(tmp_path, "gemm16_plan")
