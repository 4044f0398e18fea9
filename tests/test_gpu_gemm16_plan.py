"""Every kernel family the 16-bit GEMM plan (csrc/gemm16_plan.h) can name, launched and held to an EXACT answer.

Operands are the small integers of tests/decode_gemm_util.py: exact in bf16 and fp16, every partial sum an integer below 2^24, so the
fp32 accumulator of ANY family in ANY K order is the int64 product, and every output (+ integer bias, + integer residual) is an
integer of magnitude <= 256 that bf16 and fp16 hold exactly (tests/test_decode_gemm_host.py proves both on the CPU).  Each launch must
therefore equal the int64 expectation bit for bit, and the families must equal each other on the same operands; `info` of each launch
says which family ran.  The refusals of the plan come back as MGEA_EINVAL (RuntimeError) and launch nothing."""
import functools

import pytest
import torch

import decode_gemm_util as U

pytestmark = pytest.mark.gpu

G16_SMALL, G16_RING, G16_PERSISTENT, G16_DUO = 0, 1, 2, 3
# (switch, value) -> the family a bias epilogue gets at a shape the LDS-DMA kernels take; the residual epilogue differs under tile 5:
# the two-workgroups-per-CU kernel has none, a ring kernel runs
FORCED = [(("bf16_gemm_tile", 1), G16_RING), (("bf16_gemm_tile", 2), G16_RING), (("bf16_gemm_tile", 3), G16_RING),
          (("bf16_gemm_tile", 4), G16_PERSISTENT), (("bf16_gemm_tile", 5), G16_DUO), (("bf16_gemm_small", 1), G16_SMALL)]


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """device operands and the expected outputs (int64 product rounded once to bf16: no rounding happens) of one shape"""
    assert (M, N, K) in U.GEMM16_SHAPES
    a, w, b, r = U.int_a(M, K), U.int_w(N, K), U.int_bias(N), U.int_res(M, N)
    want = {"bias": U.int_product(a, w, b), "res": U.int_product(a, w, b, r)}
    for v in want.values():
        assert torch.equal(v.float().bfloat16().long(), v)
    return dict(a=a.bfloat16().cuda(), w=w.bfloat16().cuda(), b=b.float().cuda(), r=r.bfloat16().cuda(),
                want={k: v.float().bfloat16().cuda() for k, v in want.items()})


def launch(c, mode, dtype=torch.bfloat16):
    from mgea import ops
    info = []
    M, N = c["a"].shape[0], c["w"].shape[0]
    out = torch.full((M, N), 7.0, dtype=dtype, device="cuda")
    ops.gemm_bf16(c["a"], c["w"], c["b"], c["r"] if mode == "res" else None, info=info, out=out)
    return out, info


def test_small_shape_runs_the_register_staged_kernel():
    c = case(128, 128, 64)
    for mode in ("bias", "res"):
        got, info = launch(c, mode)
        assert info == [G16_SMALL, 0]
        assert torch.equal(got, c["want"][mode])


@pytest.mark.parametrize("mode", ["bias", "res"])
@pytest.mark.parametrize("M,N,K", [(512, 256, 64), (1000, 512, 128)])      # two tiles of 256 x 256; ragged M, two K-tiles
def test_every_family_gives_the_integer_product(M, N, K, mode, tune):
    c = case(M, N, K)
    want = c["want"][mode]
    got, info = launch(c, mode)
    assert info == [G16_RING, 0]                                           # no switch: the 256 x 128 ring kernel
    assert torch.equal(got, want)
    outs = {"default": got}
    for (switch, value), family in FORCED:
        tune(switch, value)
        got, info = launch(c, mode)
        tune(switch, 0)
        if (switch, value) == ("bf16_gemm_tile", 5) and mode == "res":
            family = G16_RING
        assert info[0] == family, (switch, value, info)
        assert torch.equal(got, want), (switch, value)
        outs[(switch, value)] = got
    for k, v in outs.items():
        assert torch.equal(v, outs["default"]), k                          # and between the families


def test_wide_ring_kernel_through_the_shape_branch(tune):
    """512 tiles of 256 x 256 with N % 256 == 0: the <4, 2> ring kernel by the shape, which only the residual epilogue under
    bf16_gemm_tile = 5 reaches while the default switches send such shapes to the persistent kernel"""
    M, N, K = 8192, 4096, 64
    c = case(M, N, K)
    tune("bf16_gemm_tile", 5)
    got, info = launch(c, "res")
    assert info == [G16_RING, 0]
    assert torch.equal(got, c["want"]["res"])
    tune("bf16_gemm_tile", 3)                                              # the same instantiation by its own switch value
    again, info = launch(c, "res")
    assert info == [G16_RING, 0] and torch.equal(again, got)
    tune("bf16_gemm_tile", 0)
    pers, info = launch(c, "res")
    assert info[0] == G16_PERSISTENT and torch.equal(pers, got)


def test_fp16_operands_run_the_persistent_kernel(tune):
    from mgea import ops
    M, N, K = 2048, 256, 64
    c = case(M, N, K)
    a, w = c["a"].half(), c["w"].half()
    info = []
    head = ops.gemm_f16_ln(a, w, c["b"], f32_out=True, info=info)          # epilogue 6: fp32 output
    assert info[0] == G16_PERSISTENT
    assert head.dtype == torch.float32 and torch.equal(head, c["want"]["bias"].float())
    # epilogue 5 with the identity tables (mean 0, rstd 1, gamma 1, beta 0): A W^T + bias + res
    ident = torch.tensor([0.0, 1.0], device="cuda").repeat(M, 1)
    ln = dict(rowstat=ident, g=torch.ones(N, device="cuda"), b=torch.zeros(N, device="cuda"))
    info = []
    got = ops.gemm_f16_ln(a, w, c["b"], c["r"].half(), ln=ln, info=info)
    assert info[0] == G16_PERSISTENT
    assert got.dtype == torch.float16 and torch.equal(got, c["want"]["res"].half())
    # ... and the bf16 instantiation of the same epilogue on the same operands (8 tiles: the persistent kernel by its switch only)
    tune("bf16_gemm_tile", 4)
    info = []
    same = ops.gemm_bf16(c["a"], c["w"], c["b"], c["r"], ln=ln, info=info)
    assert info[0] == G16_PERSISTENT and torch.equal(same.float(), got.float())


def _z(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


REFUSALS = {
    # name: (f16, M, N, K, epi, residual, ln entries or None, switches)
    "lnfold_n_not_256": (False, 32768, 384, 768, 3, False, ("rowstat", "c1"), {}),
    "k_96": (False, 32768, 768, 96, 0, False, None, {}),
    "lnfold_on_a_ring_kernel": (False, 32768, 768, 768, 3, False, ("rowstat", "c1"), {"bf16_gemm_tile": 1}),
    "bias_res_without_residual": (False, 512, 256, 64, 2, False, None, {}),
    "fp32_output_with_bf16": (False, 32768, 768, 768, 6, False, None, {}),
    "res_ln_without_rowstat": (False, 32768, 768, 768, 5, True, ("g", "b"), {}),
    "res_ln_without_gamma": (False, 32768, 768, 768, 5, True, ("rowstat", "b"), {}),
    "res_ln_without_beta": (False, 32768, 768, 768, 5, True, ("rowstat", "g"), {}),
    "lnfold_without_c1": (False, 32768, 768, 768, 3, False, ("rowstat",), {}),
    "fp16_two_tiles": (True, 512, 256, 64, 3, False, ("rowstat", "c1"), {}),
    "fp16_plain_bias": (True, 2048, 256, 64, 0, False, None, {}),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_of_the_plan_are_einval_and_launch_nothing(name, tune):
    from mgea import ops
    f16, M, N, K, epi, residual, present, switches = REFUSALS[name]
    dt = torch.float16 if f16 else torch.bfloat16
    a, w, b = _z(M, K, dtype=dt), _z(N, K, dtype=dt), _z(N, dtype=torch.float32)
    r = _z(M, N, dtype=dt) if residual else None
    ln = None
    if present is not None:
        full = dict(rowstat=_z(M, 2, dtype=torch.float32), c1=_z(N, dtype=torch.float32), g=_z(N, dtype=torch.float32), b=_z(N, dtype=torch.float32))
        keys = ("rowstat", "c1") if epi in (3, 4) else ("rowstat", "g", "b")
        ln = {k: (full[k] if k in present else None) for k in keys}
    for k, v in switches.items():
        tune(k, v)
    out = torch.full((M, N), 7.0, dtype=dt, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        (ops.gemm_f16_ln if f16 else ops.gemm_bf16)(a, w, b, r, ln=ln, epi=epi, out=out)
    assert type(ei.value) is RuntimeError, f"MGEA_EINVAL expected, got {ei.value!r}"      # (MgeaError = a HIP / other failure)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched something"
