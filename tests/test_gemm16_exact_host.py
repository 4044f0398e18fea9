"""The premises of tests/test_gpu_gemm16_exact.py, proved on the CPU for every case it launches: the reference alone never fails a
case.  Every expected value -- and every value a kernel rounds to 16 bits on the way: the accumulator and acc + bias of the residual
epilogues -- survives a round trip through the output type bit for bit; every partial sum and every epilogue intermediate is an
integer (or half of one) far below 2^24; the probe columns reach every k; the LayerNorm tables are not the identity; and under 1 % of
the GELU outputs have more than one admissible value."""
import pytest
import torch

import gemm16_exact_util as X


def _round_trips(v, dtype, what):
    assert torch.equal(v.to(torch.float32).to(dtype).to(torch.float64).long(), v), f"{what} is not exact in {dtype}"


def test_the_case_list_names_every_shape_once():
    shp = X.shapes()
    assert len(shp) == len(set(shp))
    for M, N, K, _, _ in X.exact_cases() + X.gelu_cases():
        assert (M, N, K) in shp and K % 64 == 0 and K // 64 >= 3          # past one wrap of a two-stage ring at the least
    assert {K // 64 for K in X.DEPTH_K} == {3, 4, 5, 12, 48}


@pytest.mark.parametrize("M,N,K", X.shapes())
def test_operands_and_partial_sums(M, N, K):
    c = X.case(M, N, K)
    for t in (c["a"], c["w"]):
        assert int(t.min()) == -1 and int(t.max()) == 1                    # ternary: exact in bf16 and fp16, products in {-1, 0, 1}
    assert K < 2 ** 24                                                     # so every partial sum, in any order, is an integer <= K
    assert torch.equal(c["w"].sum(1), c["c1"]) and torch.equal(c["c1"], torch.arange(N) % 9 - 4)
    assert int(c["acc"].abs().max()) <= 256                                # the accumulator itself is a bf16 value
    # dense: a single k carries a nonzero product in about 4 / 9 of the outputs (the rebalancing zeroes a few entries of W)
    dens = float((c["a"] != 0).double().mean()) * float((c["w"] != 0).double().mean())
    assert 0.36 < dens < 0.47, dens
    # even tables where the recipe says so, and not the identity: at least a third of the rows / columns each
    for k in ("res", "beta", "c2"):
        assert bool((c[k] % 2 == 0).all())
    assert set(c["mean"].tolist()) == {-1, 0, 1} and set(c["rstd"].tolist()) == {1, 2} and set(c["gamma2"].tolist()) == {1, 2, 4}
    assert float((c["mean"] != 0).double().mean()) >= 1 / 3
    assert float((c["rstd"] != 1).double().mean()) >= 1 / 3
    assert float((c["gamma2"] != 2).double().mean()) >= 1 / 3


@pytest.mark.parametrize("M,N,K,dtype,epi", X.exact_cases(), ids=str)
def test_expected_values_are_exact_in_the_output_type(M, N, K, dtype, epi):
    c = X.case(M, N, K)
    want = X.expect(c, epi)
    big = int(want.abs().max())
    print(f"[gemm16 exact] M={M} N={N} K={K} {dtype} epi {epi}: max |acc| {int(c['acc'].abs().max())}, max |want| {big}")
    if epi == 6:
        assert big < 2 ** 24                                               # fp32 output
        return
    _round_trips(want, dtype, "the expected output")
    if epi in (2, 5):                                                      # the residual epilogues round acc (persistent kernel) or
        _round_trips(c["acc"], dtype, "acc")                               # acc + bias (ring, small) to 16 bits before the residual
        _round_trips(X.pre_activation(c, epi), dtype, "acc + bias")
    if epi == 3:       # rstd * fma(-mean, c1, acc) + c2: integers
        assert int((c["acc"] - c["mean"][:, None] * c["c1"][None, :]).abs().max()) * 2 + 6 < 2 ** 24
    if epi == 5:       # fma(fma(res, rstd, -mean rstd), gamma, bias + beta): integers, then halves of even integers
        t = (c["res"] - 2 * c["mean"][:, None]) * c["rstd"][:, None]
        assert bool((t % 2 == 0).all()) and int(t.abs().max()) * 2 + int((c["bias"] + c["beta"]).abs().max()) + big < 2 ** 24
        s, m2 = X.tile_stats(want)
        assert int(s.abs().max()) <= 256 * big < 2 ** 24                   # the tile sums: fp32 sums of integers, exact in any order
        assert bool((m2 >= 0).all())


def test_probe_columns_reach_every_k_and_stay_below_256():
    M, N, K = X.PROBE_SHAPE
    p = X.probe_case(M, N, K)
    pos = p["pos"]
    assert 8 * N >= K and len(set(pos.reshape(-1).tolist())) == K          # every k of the shape, at least once
    assert all(len(set(r)) == 8 for r in pos.tolist())                     # eight DIFFERENT positions per column: weights never add up
    assert torch.equal((p["w"] != 0).sum(1), torch.full((N,), 8)) and int(p["w"].max()) == 128
    assert 0 <= int(p["want"].min()) and int(p["want"].max()) <= 255
    _round_trips(p["want"], torch.bfloat16, "the probe output")
    # the blame is right: drop k = 777 from the product and read it back from the wrong outputs
    a = p["a"].clone()
    a[:, 777] = 0
    n_wrong, lost, doubled = X.probe_blame(p, X.exact_matmul(a, p["w"]))
    assert n_wrong > 0 and lost == [777] and doubled == []
    n_wrong, lost, doubled = X.probe_blame(p, p["want"] + X.exact_matmul(p["a"][:, 64:128], p["w"][:, 64:128]))
    assert doubled == sorted(set(range(64, 128)) & set(pos.reshape(-1).tolist())) and lost == []


@pytest.mark.parametrize("M,N,K,dtype,epi", X.gelu_cases(), ids=str)
def test_gelu_intervals_are_almost_always_one_value(M, N, K, dtype, epi):
    c = X.case(M, N, K)
    pre = X.pre_activation(c, epi)
    assert int(pre.abs().max()) < 2 ** 24
    lo, hi = X.gelu_bounds(pre, dtype)
    assert bool((lo <= hi).all())
    share = float((lo != hi).double().mean())
    flat = float((pre <= -3).double().mean())
    print(f"[gemm16 gelu] M={M} N={N} K={K} {dtype} epi {epi}: {share:.3%} of the elements have more than one admissible value "
          f"({flat:.3%} with a pre-activation <= -3)")
    assert share < 0.01
    # the interval is no tighter than the type: the rounded reference itself is admissible everywhere
    g = X.gelu64(pre.double()).to(dtype)
    assert bool(((lo <= g) & (g <= hi)).all())
