"""The premises tests/test_gpu_decode_gemm.py rests on, proved on the CPU: the integer operands give fp32-exact results at every shape
used, the fp16-weight model reference equals an independent scalar evaluation, and the host page-image builder keeps the poison where
no token lands and drops positions past the table."""
import numpy as np
import pytest
import torch

import decode_gemm_util as U
from mgea import ops


def test_integer_operands_stay_below_2_pow_24_at_every_shape_used():
    shapes = U.exact_shapes()
    assert len(shapes) > 40
    for M, N, K in shapes:
        assert K <= 4096
        a, w = U.int_a(M, K), U.int_w(N, K)
        assert int(a.abs().max()) <= 3 and int(w.abs().max()) <= 8
        # the worst partial sum of ANY order is bounded by the sum of the magnitudes
        worst = int((a.abs().double() @ w.abs().double().t()).max())
        assert worst <= 24 * K <= 98304
        lift = torch.zeros(N, dtype=torch.long)
        lift[U.head_dups(N)] = U.LIFT
        total = worst + int(U.int_bias(N).abs().max()) + int(U.int_res(M, N).abs().max()) + U.LIFT
        assert total < 2 ** 24, (M, N, K, total)
        # exact in fp32 and in fp16 as stored
        assert torch.equal(a.float().half().long(), a) and torch.equal(w.float().half().long(), w)
        out = U.int_product(a, w, U.int_bias(N) + lift, U.int_res(M, N))
        assert torch.equal(out.float().long(), out)


def test_integer_operands_give_16_bit_outputs_without_rounding_at_the_gemm16_shapes():
    """tests/test_gpu_gemm16_plan.py: operands exact in bf16 and fp16 (float -> bfloat16 -> float is the identity), every partial sum in
    ANY order an integer below 2^24, and every OUTPUT (+ bias + residual) an integer of magnitude <= 256 -- exact in bf16's 8
    significant bits and in fp16: the expected output, "the int64 product rounded once", involves no rounding at all, whichever
    intermediate a kernel's epilogue stages in 16 bits."""
    for M, N, K in U.GEMM16_SHAPES:
        a, w, b, r = U.int_a(M, K), U.int_w(N, K), U.int_bias(N), U.int_res(M, N)
        for t in (a, w, r):
            assert torch.equal(t.float().bfloat16().float().long(), t) and torch.equal(t.float().half().float().long(), t)
        worst = int((a[:7].abs().double() @ w[:17].abs().double().t()).max())          # (both operands are periodic: 7 rows, 17 columns)
        assert worst + int(b.abs().max()) + int(r.abs().max()) < 2 ** 24
        for out in (U.int_product(a, w), U.int_product(a, w, b), U.int_product(a, w, b, r)):
            assert int(out.abs().max()) <= 256
            assert torch.equal(out.float().bfloat16().float().long(), out) and torch.equal(out.float().half().float().long(), out)


@pytest.mark.parametrize("K", sorted({k for _, _, k in U.exact_shapes()}))
def test_integer_operands_give_the_same_fp32_bits_in_three_summation_orders(K):
    """Both operands are periodic (A in m with period 7, W in n with period 17): 8 rows x 18 columns hold every (row, column) pattern
    of any shape.  Sequential, reversed and the kernel's wave-split order, one fp32 addition at a time, against the int64 product."""
    a, w = U.int_a(8, K), U.int_w(18, K)
    want = U.int_product(a, w).float()
    for got in U.fp32_sum_orders(a, w):
        assert torch.equal(got, want)
    # the same evaluation of operands that are NOT exact differs between the orders: the comparison can fail
    x, y = U.rnd(8, K, seed=1), U.rnd(18, K, seed=2)
    s = U.fp32_sum_orders(x, y)
    assert not (torch.equal(s[0], s[1]) and torch.equal(s[0], s[2]))


def test_operands_depend_on_each_index():
    a, w = U.int_a(14, 64), U.int_w(34, 64)
    assert len({tuple(r.tolist()) for r in a[:7]}) == 7 and len({tuple(r.tolist()) for r in w[:17]}) == 17
    assert len({tuple(c.tolist()) for c in a.t()[:7]}) == 7 and len({tuple(c.tolist()) for c in w.t()[:17]}) == 17
    # a dropped k-step (256 columns), a doubled one, and a swapped column pair each move the product by at least 1
    a, w = U.int_a(2, 1280), U.int_w(40, 1280)
    full = U.int_product(a, w)
    assert bool((U.int_product(a[:, :1024], w[:, :1024]) != full).any())
    wp = w.clone()
    wp[[3, 4]] = w[[4, 3]]
    assert bool((U.int_product(a, wp) != full).any())


def test_few_wave_shapes_take_the_wave_counts_the_tests_expect():
    assert {k: U.pick_waves(k) for k in U.FEW_WAVE_K} == U.FEW_WAVE_K
    assert U.pick_waves(512) == 8 and U.pick_waves(256) == 8 and U.pick_waves(768) == 8


@pytest.mark.parametrize("K", [256, 768])
def test_f16_model_reference_equals_a_scalar_evaluation(K):
    M, N = 3, 24
    x, w, b, g, be = U.ln_operands(M, N, K, seed=40)
    ref = U.f16_model64(x, w, b, g, be)
    for m, n in [(0, 0), (1, 7), (2, 23), (2, 16)]:
        slow = U.f16_model_slow(x, w, b, g, be, m, n)
        assert abs(float(ref[m, n]) - slow) < 1e-12, (m, n)
    # and it is a model of LN(x) W^T + b: within the fp16 rounding of W and gamma x (2^-11 relative per operand), far outside fp32 noise
    true = U.ln_gemm64(x, w, b, g, be)
    d = float((ref - true).abs().max())
    assert 1e-6 < d < 5e-3, d


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_page_image_builder_keeps_poison_and_drops_positions_past_the_table(dtype):
    H, dh, max_pages, B, T = 2, 32, 2, 3, 3
    C = H * dh
    n_pages, n_layers, layer = 7, 2, 1
    table = U.permuted_table(B, max_pages, n_pages, mult=3, add=2)
    ctx = [62, 64 * max_pages, 126]            # row 0 crosses a page, row 1 is past the table, row 2 runs off its last page
    lens = [3, 3, 2]
    qkv = U.rnd(B * T, 3 * C, seed=5)
    img = U.expected_image(ops, qkv, H, dh, table, ctx, lens, T, n_pages, layer, n_layers, dtype)
    per = ops.kv_page_elems(n_pages, H, dh)
    bits, pz = U.int_bits(img), U.int_bits(ops.poison(1, dtype))[0]
    assert bool((bits[:per] == pz).all()), "the other layer was written"
    written = int((bits[per:] != pz).sum())
    assert written == (3 + 0 + 2) * 2 * C, "tokens past the table (or padded ones) were written, or real ones lost"
    k, v = ops.kv_pages_read(img[per:], table, 0, 65, H, dh)
    want = qkv[:, C:].to(dtype)
    assert torch.equal(U.int_bits(k[62:65].reshape(3, C)), U.int_bits(want[0:3, :C].contiguous()))
    assert torch.equal(U.int_bits(v[62:65].reshape(3, C)), U.int_bits(want[0:3, C:].contiguous()))
    assert bool((U.int_bits(k[:62].contiguous()) == pz).all())
    k2, _ = ops.kv_pages_read(img[per:], table, 2, 128, H, dh)
    assert torch.equal(U.int_bits(k2[126:128].reshape(2, C)), U.int_bits(want[6:8, :C].contiguous()))
    # physical pages no table entry names stay poison
    unused = sorted(set(range(n_pages)) - set(table.reshape(-1).tolist()))
    assert unused and bool((bits[per:].view(n_pages, -1)[unused] == pz).all())
    with pytest.raises(AssertionError):
        U.permuted_table(2, 2, 4, mult=2)


def test_poison_is_a_nan_in_both_widths():
    assert bool(ops.poison(4).isnan().all()) and bool(ops.poison(4, torch.float16).isnan().all())
    assert int(U.int_bits(ops.poison(1))[0]) == ops.POISON_BITS


def test_decode_gemm_struct_matches_the_header():
    """field order and types of mgea_decode_gemm_args in include/mgea.h against the ctypes mirror"""
    import os
    import re
    from mgea import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgea.h")).read()
    body = re.search(r"typedef struct mgea_decode_gemm_args \{(.*?)\} mgea_decode_gemm_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _lib.DecodeGemmArgs._fields_]
    assert int(re.search(r"#define MGEA_DECODE_GEMM_PLAN_INTS (\d+)", src).group(1)) == _lib.DECODE_GEMM_PLAN_INTS == len(ops.PLAN_KEYS)
    assert (U.EPI_QKV, U.EPI_RES, U.EPI_ACT, U.EPI_LOGITS) == (_lib.EPI_QKV, _lib.EPI_RES, _lib.EPI_ACT, _lib.EPI_LOGITS)
    assert (U.DG_SKINNY, U.DG_HEAD, U.DG_GEMV) == (_lib.DG_SKINNY, _lib.DG_HEAD, _lib.DG_GEMV)
