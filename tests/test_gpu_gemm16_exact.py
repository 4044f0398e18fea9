"""The 16-bit GEMM families of csrc/gemm16.hip held to EXACT answers where their hand-built machinery works: K loops deep enough for
every stage ring to wrap and be refilled (3 .. 48 K-tiles), the persistent kernel streaming across tiles and into half units, fp16
instantiations, outputs and weights that are slices of wider buffers as the engines launch them, and the reversed tile walk.

Operands, expectations and the case list are tests/gemm16_exact_util.py (tests/test_gemm16_exact_host.py proves on the CPU that every
expectation is exact in the output type).  Every launch goes through ops.gemm16 (mgea_op_gemm16), asserts `info` first -- family,
half tiles, tail word -- writes into a buffer pre-filled with ops.poison that has one more row than the output, and must leave the int64
expectation bit for bit and the poison around it untouched.  Since every family must equal the same expectation they equal each other.
No tolerance anywhere except the M2 statistic of epilogue 5 (the 1e-4 of tests/test_gpu_bf16.py) and the GELU interval."""
import functools

import pytest
import torch

import gemm16_exact_util as X

pytestmark = pytest.mark.gpu

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
BITS = {BF: torch.int16, HF: torch.int16, F32: torch.int32}
SMALL, RING, PERS, DUO = X.G16_SMALL, X.G16_RING, X.G16_PERSISTENT, X.G16_DUO
# name -> ((switch, value) or None, family of a bias epilogue at a shape the LDS-DMA kernels take)
FAMILIES = {"small": (("bf16_gemm_small", 1), SMALL), "ring<2,1>": (("bf16_gemm_tile", 1), RING), "ring<2,2>": (("bf16_gemm_tile", 2), RING),
            "ring<4,2>": (("bf16_gemm_tile", 3), RING), "default": (None, RING), "duo": (("bf16_gemm_tile", 5), DUO),
            "persistent": (("bf16_gemm_tile", 4), PERS)}
PHASES, TAILS = (4, 2, 1), (0, 1, 2)


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def dev(M, N, K, dtype):
    """the device operands of X.case(M, N, K) in one 16-bit type"""
    c = X.case(M, N, K)
    f = lambda t: t.float().cuda()
    return dict(c=c, a=c["a"].to(dtype).cuda(), w=c["w"].to(dtype).cuda(), res=c["res"].to(dtype).cuda(),
                bias={e: X.bias_for(c, e).cuda() for e in range(7)}, rowstat3=X.rowstat3(c).cuda(), rowstat5=X.rowstat5(c).cuda(),
                c1=f(c["c1"]), gamma=X.gamma(c).cuda(), beta=f(c["beta"]))


@functools.lru_cache(maxsize=None)
def want(M, N, K, dtype, epi):
    """X.expect on the device in the output type (fp32 for epilogue 6): no rounding happens (host test)"""
    return X.expect(X.case(M, N, K), epi).to(F32 if epi == 6 else dtype).cuda()


class Buf:
    """[rows + 1, width] of poison; `out` = rows x N of it from column col0"""

    def __init__(self, rows, N, dtype, width=None, col0=0):
        from mgea import ops
        width = N if width is None else width
        flat = ops.poison((rows + 1) * width, F32 if dtype == F32 else HF, device="cuda")
        self.full = flat.view(dtype).reshape(rows + 1, width)
        self.bits = self.full.view(BITS[dtype])
        self.poison = int(self.bits[0, 0])
        self.rows, self.N, self.col0 = rows, N, col0
        self.out = self.full[:rows, col0:col0 + N]

    def refill(self):
        self.bits.fill_(self.poison)
        return self.out

    def check(self, expected, what):
        got = self.out.view(BITS[self.out.dtype])
        exp = expected.view(BITS[expected.dtype])
        if not torch.equal(got, exp):
            bad = torch.nonzero(got != exp)
            first = bad[:4].tolist()
            raise AssertionError(f"{what}: {bad.shape[0]} of {exp.numel()} outputs differ; rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, "
                                 f"columns {int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first {first}: got "
                                 f"{[float(self.out[m, n]) for m, n in first]} want {[float(expected[m, n]) for m, n in first]}")
        r, c0, c1 = self.rows, self.col0, self.col0 + self.N
        for name, region in (("the row behind the output", self.bits[r:]), ("the columns before it", self.bits[:r, :c0]),
                             ("the columns behind it", self.bits[:r, c1:])):
            assert bool((region == self.poison).all()), f"{what}: {name} written"


def operands(d, epi, cols=slice(None)):
    """bias / residual / LayerNorm arguments of ops.gemm16 for an epilogue; cols: the rows of the stacked weight a launch uses"""
    kw = dict(bias=d["bias"][epi][cols], epi=epi)
    if epi in (3, 4):
        kw["ln"] = dict(rowstat=d["rowstat3"], c1=d["c1"][cols])
    if epi == 5:
        kw["ln"] = dict(rowstat=d["rowstat5"], g=d["gamma"][cols], b=d["beta"][cols])
    return kw


def run(d, epi, buf, expect_info, what, cols=slice(None), **kw):
    """one launch into the refilled buffer, `info` asserted; kw replaces arguments of ops.gemm16"""
    from mgea import ops
    info = []
    args = operands(d, epi, cols)
    if epi in (2, 5):
        args["res"] = d["res"]
    args.update(kw)
    ret = ops.gemm16(args.pop("a", d["a"]), args.pop("w", d["w"]), out=buf.refill(), info=info, **args)
    assert info == list(expect_info), f"{what}: info {info}, expected {list(expect_info)}"
    return ret


def pers_info(M, N, tail, reverse=False):
    return [PERS, X.half_tiles(M, N, n_cu(), tail), tail | (4 if reverse else 0)]


def each_persistent(tune, phases=PHASES, tails=TAILS):
    for ph in phases:
        tune("bf16_gemm_phases", ph)
        for tail in tails:
            tune("bf16_gemm_tail", tail)
            yield ph, tail


def each_family(tune, M, N, epi, names=tuple(FAMILIES)):
    """(name, family the plan must report) with the family's switch set, one after the other"""
    for name in names:
        switch, family = FAMILIES[name]
        if switch:
            tune(*switch)
        if name == "duo" and epi == 2:
            family = RING                                                  # the two-workgroups-per-CU kernel has no residual epilogue
        if name == "default" and N % 256 == 0 and -(-M // 256) * (N // 256) >= 192:
            family = PERS                                                  # by the shape: 192 tiles of 256 x 256 or more
        yield name, family
        if switch:
            tune(switch[0], 0)


# ---- depth ----------------------------------------------------------------------------------------------------------------------
def all_families_exact(M, N, K, epi, tune, names=tuple(FAMILIES)):
    d, w_, buf = dev(M, N, K, BF), want(M, N, K, BF, epi), Buf(M, N, BF)
    for name, family in each_family(tune, M, N, epi, names):
        if family == PERS:
            for ph, tail in each_persistent(tune):
                what = f"persistent phases {ph} tail {tail} ({M}, {N}, {K}) epi {epi}"
                run(d, epi, buf, pers_info(M, N, tail), what)
                buf.check(w_, what)
        else:
            what = f"{name} ({M}, {N}, {K}) epi {epi}"
            run(d, epi, buf, [family, 0, 0], what)
            buf.check(w_, what)


@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("K", X.DEPTH_K)
def test_depth_every_family_and_instantiation(K, epi, tune):
    """3 .. 48 K-tiles on the ring kernels <2, 1>, <2, 2> (by its switch and by default), <4, 2>, the two-workgroups-per-CU kernel and the
    persistent kernel in its three K loops x three tail schedules"""
    all_families_exact(*X.RING_MN, K, epi, tune, names=[n for n in FAMILIES if n != "small"])


@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("K", X.DEPTH_K)
def test_depth_small_kernel(K, epi):
    M, N = X.SMALL_MN
    buf = Buf(M, N, BF)
    what = f"small ({M}, {N}, {K}) epi {epi}"
    run(dev(M, N, K, BF), epi, buf, [SMALL, 0, 0], what)                   # by its shape: M < 512
    buf.check(want(M, N, K, BF, epi), what)


@pytest.mark.parametrize("epi", [0, 2])
def test_ragged_last_column_tile(epi, tune):
    """N = 384: one and a half column tiles of 256, three of 128 -- every family clamps its W rows and must not store past column N"""
    all_families_exact(*X.RAGGED, epi, tune)


def test_duo_reuses_ring_and_c_stage(tune):
    """528 tiles of 256 x 128 on at most 512 workgroups: some take a second tile through the same A stages and W buffer"""
    M, N, K = X.DUO_REUSE
    assert -(-M // 256) * (N // 128) == 528
    tune("bf16_gemm_tile", 5)
    buf = Buf(M, N, BF)
    run(dev(M, N, K, BF), 0, buf, [DUO, 0, 0], "duo, 528 tiles")
    buf.check(want(M, N, K, BF, 0), "duo, 528 tiles")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bit_probes_name_the_k(family, tune):
    """K = 3072 with one-hot-weighted columns: on a mismatch the message names the k's that were lost or doubled"""
    from mgea import ops
    M, N, K = X.PROBE_SHAPE
    p = X.probe_case(M, N, K)
    a, w, w_ = p["a"].to(BF).cuda(), p["w"].to(BF).cuda(), p["want"].to(BF).cuda()
    for _, fam in each_family(tune, M, N, 0, [family]):
        buf, info = Buf(M, N, BF), []
        ops.gemm16(a, w, out=buf.refill(), info=info)
        assert info[0] == fam, info
        if not torch.equal(buf.out, w_):
            n_wrong, lost, doubled = X.probe_blame(p, buf.out.float().nan_to_num(-1.0).cpu().long())
            print(f"[gemm16 probe] {family}: {n_wrong} wrong outputs; lost k {lost}; doubled k {doubled}")
            raise AssertionError(f"{family}: {n_wrong} wrong outputs; lost k {lost[:64]}; doubled k {doubled[:64]}")
        buf.check(w_, f"probe {family}")


# ---- the persistent kernel across tiles and half units ---------------------------------------------------------------------------
def check_stats(stats, w_int, what):
    s, m2 = X.tile_stats(w_int)
    got = stats.cpu()
    assert torch.equal(got[..., 0], s.float()), f"{what}: tile sums differ from the host's"
    err = float(((got[..., 1].double() - m2).abs() / (m2 + 1)).max())
    print(f"[gemm16 exact] {what}: tile M2 rel {err:.2e} (1e-4)")
    assert err < 1e-4, f"{what}: tile M2 off by {err:.3e} of (M2 + 1)"


def persistent_exact(M, N, K, dtype, epi, tune, phases=PHASES, tails=TAILS):
    from mgea import ops
    d, w_, buf = dev(M, N, K, dtype), want(M, N, K, dtype, epi), Buf(M, N, F32 if epi == 6 else dtype)
    for ph, tail in each_persistent(tune, phases, tails):
        what = f"persistent {dtype} phases {ph} tail {tail} ({M}, {N}, {K}) epi {epi}"
        kw = {}
        if epi == 5:
            stats = ops.poison(M * (N // 256) * 2, F32, device="cuda").reshape(M, N // 256, 2)
            kw["ln"] = dict(operands(d, 5)["ln"], stats=stats)
        run(d, epi, buf, pers_info(M, N, tail), what, **kw)
        buf.check(w_, what)
        if epi == 5:
            check_stats(stats, X.expect(d["c"], 5), what)


@pytest.mark.parametrize("epi", [0, 2, 3, 5])
@pytest.mark.parametrize("M,N,K", X.STREAM)
def test_persistent_streams_across_tiles_and_half_units(M, N, K, epi, tune):
    """272 / 306 tiles on at most 256 workgroups: a second whole tile streamed into (tail 0; 3 and 5 K-tiles flip the stage parity) or
    half units whose three-stage loop wraps (tails 1, 2); M % 256 == 128 at (8576, 2304, 768): no lower half behind row M"""
    assert X.half_tiles(M, N, 256, 1) == 1 and X.half_tiles(M, N, 256, 0) == 0
    persistent_exact(M, N, K, BF, epi, tune)


@pytest.mark.parametrize("epi", [3, 5, 6])
@pytest.mark.parametrize("M,N,K", X.F16_SHAPES)
def test_fp16_instantiations(M, N, K, epi, tune):
    persistent_exact(M, N, K, HF, epi, tune)


# ---- strided, as the engines launch it ------------------------------------------------------------------------------------------
STRIDED = [(BF, 0, name) for name in FAMILIES] + [(BF, 3, "persistent"), (HF, 3, "persistent")]


@pytest.mark.parametrize("K", X.STRIDED_K)
@pytest.mark.parametrize("dtype,epi,family", STRIDED, ids=str)
def test_output_and_weights_are_slices_of_wider_buffers(dtype, epi, family, K, tune):
    """out = columns [D, 3D) of a poisoned [M + 1, 3D] buffer, w / bias / c1 / c2 = rows D.. of the stacked operands, N = 2D: the last
    DistilBERT layer and the decoder's K | V prefill.  Columns [0, D) and row M stay poison."""
    D, M = X.STRIDED_D, X.STRIDED_M
    d = dev(M, 3 * D, K, dtype)
    w_ = want(M, 3 * D, K, dtype, epi)[:, D:]
    cols = slice(D, 3 * D)
    buf = Buf(M, 2 * D, dtype, width=3 * D, col0=D)
    assert buf.out.stride(0) == 3 * D and d["w"][D:].data_ptr() != d["w"].data_ptr()
    for name, fam in each_family(tune, M, 2 * D, epi, [family]):          # (fp16: the persistent kernel whatever the switch)
        for ph, tail in (each_persistent(tune) if fam == PERS else [(0, 0)]):
            what = f"strided {name} {dtype} phases {ph} tail {tail} K {K} epi {epi}"
            run(d, epi, buf, pers_info(M, 2 * D, tail) if fam == PERS else [fam, 0, 0], what, cols=cols, w=d["w"][D:])
            buf.check(w_, what)


@pytest.mark.parametrize("which", ["lda", "ldw"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_operand_rows_longer_than_k(family, which, tune):
    """a (or w) = K columns out of the middle of a wider matrix whose other columns hold 3s: read, they would change every output"""
    M, N, K = *X.RING_MN, 256
    d, w_, buf = dev(M, N, K, BF), want(M, N, K, BF, 0), Buf(M, N, BF)
    src = d["a"] if which == "lda" else d["w"]
    wide = torch.full((src.shape[0], K + 128), 3.0, dtype=BF, device="cuda")
    wide[:, 64:64 + K] = src
    sl = wide[:, 64:64 + K]
    assert sl.stride(0) == K + 128 and torch.equal(sl, src)
    for name, fam in each_family(tune, M, N, 0, [family]):
        for ph, tail in (each_persistent(tune, tails=(2,)) if fam == PERS else [(0, 0)]):
            what = f"{which} = K + 128, {name} phases {ph}"
            run(d, 0, buf, pers_info(M, N, tail) if fam == PERS else [fam, 0, 0], what, **{"a" if which == "lda" else "w": sl})
            buf.check(w_, what)


def test_wrapper_refuses_what_the_plan_would():
    from mgea import ops
    M, N, K = *X.RING_MN, 256
    d = dev(M, N, K, BF)
    out = torch.zeros(M, N, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gemm16(d["a"].t().contiguous().t(), d["w"], out=out)           # inner stride != 1
    with pytest.raises(RuntimeError):
        ops.gemm16(d["a"], d["w"], res=torch.zeros(M, N + 8, dtype=BF, device="cuda")[:, :N], out=out)   # res with another row stride
    with pytest.raises(RuntimeError):
        ops.gemm16(d["a"][:, :K - 4], d["w"][:, :K - 4], out=out)          # the plan: K % 64
    torch.cuda.synchronize()
    assert not bool(out.any()), "a refused call launched something"


# ---- the reversed walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,epi", [(BF, 2), (BF, 5), (HF, 5)], ids=str)
@pytest.mark.parametrize("M,N,K", X.REVERSE)
def test_reversed_walk_is_exact_and_equals_the_forward_walk(M, N, K, dtype, epi, tune):
    """reverse = 1 as both engines launch FC2: another tile per workgroup, half units from the other end of the run and another
    candidate for the lower half that starts at row M -- the same bits"""
    d, w_ = dev(M, N, K, dtype), want(M, N, K, dtype, epi)
    fwd, rev = Buf(M, N, dtype), Buf(M, N, dtype)
    for ph, tail in each_persistent(tune, phases=(2, 1)):
        what = f"reversed {dtype} phases {ph} tail {tail} ({M}, {N}, {K}) epi {epi}"
        run(d, epi, rev, pers_info(M, N, tail, reverse=True), what, reverse=True)
        rev.check(w_, what)
        run(d, epi, fwd, pers_info(M, N, tail), what + " (forward)")
        assert torch.equal(rev.bits, fwd.bits), what + ": differs from the forward walk"
    tune("bf16_gemm_reverse", 0)
    run(d, epi, rev, pers_info(M, N, tail), "reverse asked for with bf16_gemm_reverse = 0", reverse=True)   # the bit is clear
    rev.check(w_, "bf16_gemm_reverse = 0")


# ---- GELU on an exact accumulator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,dtype,epi", X.gelu_cases(), ids=str)
def test_gelu_epilogues_on_an_exact_accumulator(M, N, K, dtype, epi, tune):
    """every output one of the 16-bit roundings of g +- 1.5e-5 max(1, |g|), g the float64 erf-GELU of the exact pre-activation"""
    d = dev(M, N, K, dtype)
    lo, hi = (t.cuda().float() for t in X.gelu_bounds(X.pre_activation(d["c"], epi), dtype))
    buf = Buf(M, N, dtype)

    def check(what):
        got = buf.out.float()
        bad = ~((lo <= got) & (got <= hi))                                 # (poison is a NaN: inside no interval)
        if bool(bad.any()):
            at = torch.nonzero(bad)[:4].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs outside their interval; first {at}: got "
                                 f"{[float(got[m, n]) for m, n in at]}, [lo, hi] {[(float(lo[m, n]), float(hi[m, n])) for m, n in at]}")
        assert bool((buf.bits[M:] == buf.poison).all()), f"{what}: the row behind the output written"

    for name, fam in each_family(tune, M, N, epi, list(FAMILIES) if epi == 1 else ["persistent"]):
        if fam == PERS:
            for ph, tail in each_persistent(tune, tails=(0, 2)):
                what = f"gelu persistent {dtype} phases {ph} tail {tail} ({M}, {N}, {K}) epi {epi}"
                run(d, epi, buf, pers_info(M, N, tail), what)
                check(what)
        else:
            what = f"gelu {name} ({M}, {N}, {K})"
            run(d, epi, buf, [fam, 0, 0], what)
            check(what)
