"""Host side of tests/test_gpu_gemm16_exact.py (proved by tests/test_gemm16_exact_host.py): operands on which the 16-bit GEMMs of
csrc/gemm16.hip have ONE right answer at any depth, the expected answers, and the list of cases the GPU test launches.  CPU torch only.

DENSE TERNARY OPERANDS.  A[m, k], W[n, k] in {-1, 0, 1} from a seeded generator, integer bias, even integer residual.  Every product
is -1, 0 or 1, every partial sum over K <= 3072 an integer of magnitude <= K < 2^24: an fp32 accumulator holds it exactly in ANY
summation order, so every kernel family, stage ring and wave split must return the int64 product.  The sum over K is a random walk
(variance 4 K / 9), far inside what bf16 holds exactly (integers to 256, even integers to 512).  One k lost or doubled moves the 4 / 9
of the outputs whose a w is not 0 by +-1; an A tile paired with another W tile, or a stale stage read twice, moves nearly all.

LAYERNORM TABLES THAT STAY EXACT (epilogues 3 / 4 / 5).  Row means in {-1, 0, 1}, rstd in {1, 2}, gamma in {0.5, 1, 2} by column,
even beta and c2, even residual; the rows of W are rebalanced -- entries of one sign zeroed -- until their sum is c1[n] = n % 9 - 4
exactly, as the fold defines c1.  Then rstd (acc - mean c1) + c2 and acc + bias + ((res - 2 mean) rstd gamma + beta) (the residual's
own mean is 2 mean: even) are integers, and so is every intermediate of the kernels' epilogues, in any association.

BIT PROBES.  A in {0, 1}; row n of W is zero except at eight positions k_0(n) .. k_7(n) with the weights 1, 2, .. 128, so
out[m, n] = sum_j 2^j A[m, k_j(n)] <= 255 and a wrong output NAMES the k's that were lost (bits cleared) or doubled (bits carried):
probe_blame().  k_j(n) = (1531 (8 n + j)) mod K: 1531 is coprime to K = 2^a 3, so 8 N >= K consecutive probes reach every k.

GELU (epilogues 1 / 4) cannot be exact, the accumulator can: the pre-activation is the integer above, and an output must be one of the
16-bit roundings of [g - t, g + t], g = the float64 erf-GELU of it, t = 1.5e-5 max(1, |g|) (the error of csrc/x16.h gelu_fast).  Where
GELU is flat the interval holds many 16-bit values (g ~ 0 for a pre-activation <= -3), which says little; the bias of these cases is
lifted by gelu_lift(K) so that fewer than 1 % of the elements have more than one admissible value."""
import functools
import math

import torch

G16_SMALL, G16_RING, G16_PERSISTENT, G16_DUO = 0, 1, 2, 3
GELU_TOL = 1.5e-5
PROBE_STEP = 1531

DEPTH_K = (192, 256, 320, 768, 3072)                  # 3, 4, 5, 12 and 48 K-tiles: odd and even counts, past both ring depths
SMALL_MN, RING_MN = (144, 256), (1000, 512)
RAGGED = (512, 384, 192)                               # a ragged last column tile for every tile width
DUO_REUSE = (8448, 2048, 192)                          # 528 tiles of 256 x 128 on at most 512 slots
STREAM = [(4352, 4096, 192), (4352, 4096, 320), (8576, 2304, 768)]
F16_SHAPES = [(1024, 512, 3072), (4352, 4096, 320)]
STRIDED_D, STRIDED_M, STRIDED_K = 256, 1024, (256, 768)
REVERSE = [(4352, 4096, 320), (8576, 2304, 768)]
GELU_SHAPES = [(1000, 512, 3072), (4352, 4096, 320)]
PROBE_SHAPE = (1000, 512, 3072)


def shapes():
    """every (M, N, K) the GPU test builds a case() for"""
    s = [(m, n, k) for m, n in (SMALL_MN, RING_MN) for k in DEPTH_K] + [RAGGED, DUO_REUSE] + STREAM + F16_SHAPES + REVERSE + GELU_SHAPES
    s += [(STRIDED_M, 3 * STRIDED_D, k) for k in STRIDED_K]
    return sorted(set(s))


def exact_cases():
    """every (M, N, K, dtype, epilogue) the GPU test holds to expect(): what the host test proves representable.  (fp16 has epilogues
    3 .. 6 only: the reversed walk runs epilogue 2 in bf16 alone.)"""
    bf, hf = torch.bfloat16, torch.float16
    s = [(m, n, k, bf, e) for m, n in (SMALL_MN, RING_MN) for k in DEPTH_K for e in (0, 2)]
    s += [(*shp, bf, e) for shp in (RAGGED, DUO_REUSE) for e in (0, 2)]
    s += [(*shp, bf, e) for shp in STREAM for e in (0, 2, 3, 5)]
    s += [(*shp, hf, e) for shp in F16_SHAPES for e in (3, 5, 6)]
    s += [(STRIDED_M, 3 * STRIDED_D, k, dt, e) for k in STRIDED_K for dt, e in ((bf, 0), (bf, 3), (hf, 3))]
    s += [(*shp, dt, e) for shp in REVERSE for dt, e in ((bf, 2), (bf, 5), (hf, 5))]
    return sorted(set(s), key=str)


def gelu_cases():
    """(M, N, K, dtype, epilogue) of the GELU test: epilogue 1 is bf16 only"""
    return [(*shp, dt, e) for shp in GELU_SHAPES for dt, e in ((torch.bfloat16, 1), (torch.bfloat16, 4), (torch.float16, 4))]


def _gen(M, N, K, salt):
    return torch.Generator().manual_seed(((M * 1009 + N) * 1013 + K) * 17 + salt)


def ternary(rows, cols, gen):
    return torch.randint(-1, 2, (rows, cols), generator=gen, dtype=torch.int64)


def rebalance(w, target, gen):
    """zero entries of one sign in every row of w (random ones, so no K-tile is singled out) until the row sums are `target`"""
    d = w.sum(1) - target                                  # > 0: zero d entries equal to +1; < 0: -d entries equal to -1
    sign = torch.sign(d)
    cand = w == sign[:, None]
    assert bool((cand.sum(1) >= d.abs()).all()), "a row has too few entries of one sign to reach its sum"
    pri = torch.rand(w.shape, generator=gen) * cand        # candidates in random order, everything else last
    order = torch.argsort(pri, dim=1, descending=True)
    kill = torch.arange(w.shape[1])[None, :] < d.abs()[:, None]
    out = w.scatter(1, order, torch.where(kill, torch.zeros_like(w), w.gather(1, order)))
    assert torch.equal(out.sum(1), target)
    return out


def exact_matmul(a, w):
    """a @ w^T as int64 (an fp64 matmul of small integers is exact and runs on BLAS)"""
    p = a.double() @ w.double().t()
    out = p.long()
    assert bool((out.double() == p).all())
    return out


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """int64 operands, tables and the accumulator of one shape.  W is the rebalanced matrix for every epilogue: one accumulator serves
    the plain and the LayerNorm epilogues of a shape."""
    assert (M, N, K) in shapes()
    m, n = torch.arange(M), torch.arange(N)
    a = ternary(M, K, _gen(M, N, K, 0))
    c1 = n % 9 - 4
    w = rebalance(ternary(N, K, _gen(M, N, K, 1)), c1, _gen(M, N, K, 2))
    c = dict(M=M, N=N, K=K, a=a, w=w, c1=c1,
             bias=(37 * n) % 23 - 11,
             res=2 * torch.randint(-4, 5, (M, N), generator=_gen(M, N, K, 3), dtype=torch.int64),
             mean=m % 3 - 1,                               # two thirds of the rows != 0
             rstd=1 + (m % 5 < 2).long(),                  # two fifths of the rows = 2
             gamma2=torch.tensor([1, 2, 4])[n % 3],        # 2 gamma: gamma = 0.5, 1, 2; two thirds of the columns != 1
             beta=2 * (n % 5 - 2), c2=2 * (n % 7 - 3))
    c["acc"] = exact_matmul(a, w)
    return c


def gelu_lift(K, rstd_max=1):
    """even bias lift of the GELU cases: 2.6 standard deviations of the accumulator's random walk + 4, so that under 1 % of the
    pre-activations are <= -3, where GELU is flat and almost any small output is admissible.  With rstd = 2 on two fifths of the rows
    (epilogue 4) it is 2.2 of THEIR standard deviations: a larger lift pushes the rstd = 1 rows past 256, where every odd integer is a
    tie of the bf16 rounding and has two admissible values."""
    return 2 * math.ceil((1.3 if rstd_max == 1 else 1.1 * rstd_max) * math.sqrt(4 * K / 9)) + 4


def pre_activation(c, epi):
    """what the epilogue's GELU / residual stage receives, int64: epilogues 0, 1, 2, 5, 6 acc + bias; 3, 4 rstd (acc - mean c1) + c2;
    the GELU epilogues with their lift"""
    if epi in (3, 4):
        lift = gelu_lift(c["K"], 2) if epi == 4 else 0
        return c["rstd"][:, None] * (c["acc"] - c["mean"][:, None] * c["c1"][None, :]) + (c["c2"] + lift)[None, :]
    return c["acc"] + (c["bias"] + (gelu_lift(c["K"]) if epi == 1 else 0))[None, :]


def ln_residual(c):
    """LayerNorm of the residual rows with the tables of epilogue 5 (mean 2 mean, rstd, gamma, beta), int64 (gamma2 = 2 gamma)"""
    t = (c["res"] - 2 * c["mean"][:, None]) * c["rstd"][:, None] * c["gamma2"][None, :]
    assert bool((t % 2 == 0).all())
    return t // 2 + c["beta"][None, :]


def expect(c, epi):
    """the one right answer of an exact epilogue (0, 2, 3, 5, 6), int64"""
    assert epi in (0, 2, 3, 5, 6)
    pre = pre_activation(c, epi)
    if epi == 2:
        return pre + c["res"]
    if epi == 5:
        return pre + ln_residual(c)
    return pre


def tile_stats(want):
    """epilogue 5's statistics of its own output: (sum, M2 about the tile's mean) of every 256-column tile -> int64 [M, N / 256] sums,
    float64 M2"""
    t = want.reshape(want.shape[0], -1, 256)
    s = t.sum(-1)
    d = t.double() - (s.double() / 256)[..., None]
    return s, (d * d).sum(-1)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_bounds(pre, dtype):
    """(lo, hi) in `dtype`: an output o is admissible iff lo <= o <= hi -- the 16-bit roundings of [g - t, g + t] are exactly the 16-bit
    values between the roundings of its ends (rounding is monotonic)"""
    g = gelu64(pre.double())
    t = GELU_TOL * g.abs().clamp(min=1.0)
    return (g - t).to(dtype), (g + t).to(dtype)


# ---- the operand tables as the kernels take them ------------------------------------------------------------------------------
def rowstat3(c):
    """epilogues 3 / 4: (mean, rstd) of the A rows, fp32 [M, 2]"""
    return torch.stack([c["mean"], c["rstd"]], 1).float()


def rowstat5(c):
    """epilogue 5: (mean, rstd) of the residual rows -- the mean is 2 mean, even like the residual"""
    return torch.stack([2 * c["mean"], c["rstd"]], 1).float()


def gamma(c):
    return c["gamma2"].float() / 2


def bias_for(c, epi):
    """the fp32 vector of the bias slot: c2 for the folded epilogues, the lift included for the GELU ones"""
    if epi in (3, 4):
        return (c["c2"] + (gelu_lift(c["K"], 2) if epi == 4 else 0)).float()
    return (c["bias"] + (gelu_lift(c["K"]) if epi == 1 else 0)).float()


# ---- bit probes -----------------------------------------------------------------------------------------------------------------
def probe_positions(N, K):
    """k_j(n), int64 [N, 8]"""
    return (PROBE_STEP * (8 * torch.arange(N)[:, None] + torch.arange(8)[None, :])) % K


@functools.lru_cache(maxsize=None)
def probe_case(M, N, K):
    a = torch.randint(0, 2, (M, K), generator=_gen(M, N, K, 4), dtype=torch.int64)
    pos = probe_positions(N, K)
    w = torch.zeros(N, K, dtype=torch.int64).scatter(1, pos, (1 << torch.arange(8))[None, :].expand(N, 8).contiguous())
    return dict(M=M, N=N, K=K, a=a, w=w, pos=pos, want=exact_matmul(a, w))


def probe_blame(p, got, limit=4096):
    """Which k's a wrong probe output blames: got - want < 0 clears the bits of lost k's, > 0 carries those of doubled ones.
    -> (n_wrong, sorted lost k's, sorted doubled k's) from the first `limit` wrong elements (got: int64 [M, N] on the CPU)"""
    bad = torch.nonzero(got != p["want"])
    lost, doubled = set(), set()
    for m, n in bad[:limit].tolist():
        d = int(got[m, n] - p["want"][m, n])
        for j in range(8):
            if (abs(d) >> j) & 1:
                (lost if d < 0 else doubled).add(int(p["pos"][n, j]))
    return bad.shape[0], sorted(lost), sorted(doubled)


# ---- the plan's half-tile rule (csrc/gemm16_plan.h gemm16_half_tiles, grid as plan_gemm16 sets it) ------------------------------
def half_tiles(M, N, n_cu, tail):
    n_tiles = -(-M // 256) * -(-N // 256)
    cu8 = n_cu // 8 * 8
    grid = (min(n_tiles, cu8) + 7) // 8 * 8
    wg_x, per_x = grid // 8, min((n_tiles + 7) // 8, n_tiles)
    rem = per_x - per_x // wg_x * wg_x
    return 1 if tail != 0 and rem > 0 and 2 * rem <= wg_x else 0
