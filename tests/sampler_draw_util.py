"""The sampler's DRAW restated on the host (tests/test_sampler_draw_host.py proves its premises on the CPU, tests/test_gpu_sampler_draw.py
holds csrc/sampler.hip to it on the MI355X): a Philox4x32-10 in plain Python integers, written from the Philox definition (Salmon et
al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and checked against the published Random123 known answers; the counter, key
and u the header documents (include/mgea.h, mgea_row_sampler); the CDF order; and the ids a float64 distribution admits for a given u.

THE RULE.  Row b draws its step-t number from
    counter = {stream, low 32 bits of t, bits 32..63 of t, 0x6d676561}       key = (low 32 bits of seed, high 32 bits of seed)
    u = (word 0 of Philox4x32-10(key, counter) >> 8) * 2^-24                  in [0, 1) on the 2^-24 grid
and takes the id whose interval [C_before, C_incl) of the normalised CDF over the kept ids holds u.  The CDF runs over the ids in
cdf_order().  A call without records draws row b from stream b.

numpy / CPU torch only, no device code."""
import numpy as np
import torch

import truncation_util as tu
from oracle.decoder_ref import DecoderRef

MASK32 = 0xFFFFFFFF
COUNTER_CONST = 0x6D676561
# the multipliers and the Weyl key increments of Philox4x32 (the SC'11 paper, table 2 and section 3.3: golden ratio and sqrt(3) - 1)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DELTA = 2e-5            # the project's fp32 row-operation bound (tests/step_tail_util.py, TOL): derived in test_gpu_sampler_draw.py
UNIQUE_SHARE = 0.85     # the input condition: at least this share of a tolerance case's draws admit exactly one id at DELTA
SAMP_NT = 256           # threads per row of the sampler: thread t owns ids t, t + 256, ...
B_DRAWS = 256           # rows (= draws) of one launch of the GPU tests


def philox4x32_10(key, ctr, rounds=10):
    """key: 2 words, ctr: 4 words -> 4 words.  One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2 as 64-bit products;
    c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between rounds."""
    k0, k1 = (int(k) & MASK32 for k in key)
    c0, c1, c2, c3 = (int(c) & MASK32 for c in ctr)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
    return c0, c1, c2, c3


def counter_words(stream, step):
    return int(stream) & MASK32, int(step) & MASK32, (int(step) >> 32) & MASK32, COUNTER_CONST


def key_words(seed):
    return int(seed) & MASK32, (int(seed) >> 32) & MASK32


def draw_u(seed, stream, step):
    """The number row (seed, stream) draws at step `step` (both 64-bit, stream a 32-bit word): a multiple of 2^-24 in [0, 1)."""
    return (philox4x32_10(key_words(seed), counter_words(stream, step))[0] >> 8) / 2 ** 24


def cdf_order(V):
    """The ids in the order the sampler's CDF runs over them, "thread-major": sorted by (id mod 256, id div 256) -- thread 0's ids
    0, 256, 512, ..., then thread 1's.  This order is THIS BUILD'S rule, like "ties to the lowest id": include/mgea.h promises only
    the distribution (any fixed order gives the same one).  A later change of order changes this one function."""
    ids = np.arange(int(V), dtype=np.int64)
    return ids[np.lexsort((ids // SAMP_NT, ids % SAMP_NT))]


def intervals(p):
    """p float64 [V] (any positive scale) -> (ids, C_before, C_incl): the ids with p > 0 in cdf_order and their intervals of the
    normalised float64 CDF; the last C_incl is exactly 1."""
    p = np.asarray(p, np.float64).reshape(-1)
    order = cdf_order(p.shape[0])
    ids = order[p[order] > 0]
    c = np.cumsum(p[ids])
    c_incl = c / c[-1]
    c_before = np.concatenate([[0.0], c_incl[:-1]])
    c_incl[-1] = 1.0
    return ids, c_before, c_incl


def admissible_range(p, us, delta):
    """Vectorised admissible(): for every u of `us` the first and the last position, in intervals(p)'s ids, of the ids it admits."""
    ids, c_before, c_incl = intervals(p)
    us = np.asarray(us, np.float64)
    if delta == 0:
        first = np.searchsorted(c_incl, us, side="right")      # the first interval with u < C_incl
        first = np.minimum(first, len(ids) - 1)
        return ids, first, first
    first = np.searchsorted(c_incl, us - delta, side="left")    # the first interval with C_incl >= u - delta
    last = np.searchsorted(c_before, us + delta, side="right") - 1   # the last one with C_before <= u + delta
    return ids, np.minimum(first, len(ids) - 1), np.maximum(last, 0)


def admissible(p, u, delta):
    """The ids with p > 0 whose CDF interval [C_before, C_incl] in cdf_order meets [u - delta, u + delta], in that order (contiguous
    among the kept ids); delta = 0: the single id with C_before <= u < C_incl."""
    ids, first, last = admissible_range(p, [u], delta)
    return ids[int(first[0]):int(last[0]) + 1]


def n_admissible(p, us, delta):
    _, first, last = admissible_range(p, us, delta)
    return last - first + 1


def distance(p, us, drawn):
    """How far every u is from the interval of the id drawn for it: 0 inside, inf for an id without mass.  An id is in
    admissible(p, u, delta) iff its distance is <= delta (delta > 0)."""
    ids, c_before, c_incl = intervals(p)
    pos = np.full(np.asarray(p).reshape(-1).shape[0], -1, np.int64)
    pos[ids] = np.arange(len(ids))
    drawn = np.asarray(drawn, np.int64)
    ok = (drawn >= 0) & (drawn < len(pos))
    at = np.where(ok, pos[np.where(ok, drawn, 0)], -1)
    us = np.asarray(us, np.float64)
    d = np.maximum(np.maximum(c_before[at] - us, us - c_incl[at]), 0.0)
    return np.where(at >= 0, d, np.inf)


# ---- counters ---------------------------------------------------------------------------------------------------------------------
STEPS = (0, 3, 1000, 2 ** 32 + 5, 2 ** 40 + 1)      # a launch has one step: case i uses STEPS[i % 5]


def counters(case_index, B):
    """The (seed, stream) of the B rows of case `case_index`, and the launch's step: seeds on both sides of 2^32, streams over the
    whole 32-bit range (2^32 - 1 among them), one of STEPS."""
    rows = []
    for b in range(B):
        seed = (0x9E3779B97F4A7C15 * (case_index + 1) + 0x0000000100000001 * b) % 2 ** 64 if b % 4 else 1000 * case_index + b
        stream = MASK32 if b == 1 else (2654435761 * b + 40503 * case_index) & MASK32
        rows.append((seed, stream))
    return rows, STEPS[case_index % len(STEPS)]


# Draws that land exactly ON a thread boundary of the exact family: u * 256 is an integer, so with n kept entries spread evenly over T
# threads (T a power of two <= 256) the draw's target equals the owner thread's exclusive prefix exactly -- the case `pre <= target`
# against `pre < target` decides.  (seed, stream) at step BOUNDARY_STEP; found by searching streams upwards from 0, one hit in 2^16.
BOUNDARY_SEED, BOUNDARY_STEP = 0x0123456789ABCDEF, 11
BOUNDARY_STREAMS = (31361, 57705, 219726, 309806, 329822, 511062)      # u * 256 = 5, 64, 248, 240, 54, 192


def boundary_counters():
    return [(BOUNDARY_SEED, s) for s in BOUNDARY_STREAMS], BOUNDARY_STEP


# ---- the exact family -----------------------------------------------------------------------------------------------------------
NINF = -np.inf


def exact_row(V, ids, value=0.0):
    x = np.full(int(V), NINF, np.float32)
    x[np.asarray(ids, np.int64)] = value
    return x


def _regs(V, regs):
    ids = np.arange(V)
    return ids[np.isin(ids // SAMP_NT, list(regs))]


# name -> (V, kept ids, top_k): n kept entries at logit 0, n a power of two; everything else -inf
EXACT_CASES = {
    "a_one_per_wave": (300, [5, 64 + 7, 128 + 9, 192 + 11], 0),
    "b_one_wave_register0": (300, list(range(64, 128)), 0),
    "c_one_thread_36": (8324, [37 + SAMP_NT * j for j in range(33) if j != 16], 0),       # registers 0 and 32, the last V reaches
    "c_one_thread_56": (14336, [200 + SAMP_NT * j for j in list(range(16)) + list(range(40, 56))], 0),
    "d_flat_8192": (8192, list(range(8192)), 0),
    "d_flat_8192_of_8324": (8324, list(range(8192)), 0),
    "e_wide_8192_of_14336": (14336, _regs(14336, list(range(16)) + list(range(40, 56))).tolist(), 0),
    "f_last_id": (8324, [8323], 0),
    "g_v40": (40, [i for i in range(40) if i % 5], 0),
    "h_all_equal_top_k_64": (8324, None, 64),      # every logit equal: the tie rule keeps ids 0..63
}


def exact_case(name):
    """(x float32 [V], kept ids int64 in cdf_order, top_k)"""
    V, ids, k = EXACT_CASES[name]
    if ids is None:
        x, ids = np.full(V, 1.25, np.float32), list(range(k))
    else:
        x = exact_row(V, ids)
    keep = np.zeros(V, bool)
    keep[np.asarray(ids)] = True
    order = cdf_order(V)
    kept = order[keep[order]]
    n = len(kept)
    assert n & (n - 1) == 0, f"{name}: {n} kept entries"
    return x, kept, k


def exact_expected(kept, us):
    """the kept id at index floor(u * n): u * n is exact in fp32 and in fp64 (u has 24 bits, n is a power of two)"""
    n = len(kept)
    return kept[np.floor(np.asarray(us, np.float64) * n).astype(np.int64)]


# ---- the tolerance family ---------------------------------------------------------------------------------------------------------
VOCABS = (40, 300, 8324, 9217, 14336)
# name -> (temperature, top_k, top_p, truncation settings of tests/truncation_util.py)
SETTINGS = {
    "untruncated": (1.0, 0, None, {}),
    "T0.9_k50": (0.9, 50, None, {}),
    "p0.9": (1.0, 0, 0.9, {}),
    "T0.7_k200_p0.5": (0.7, 200, 0.5, {}),
    "all": (1.0, 0, None, tu.CASES["all"]),
}
TOLERANCE_CASES = [(V, None, s) for V in VOCABS for s in SETTINGS] + [(8324, 3.0, s) for s in SETTINGS]   # scale None: logit_scale(V)
# ... and the flatter row every entry point of the sampler is run on (test_every_instantiation_draws_by_the_rule), at both kernel widths
ENTRY_TOLERANCE = {8324: (8324, 3.0, "p0.9"), 14336: (14336, 3.0, "T0.9_k50")}
TOLERANCE_CASES.append(ENTRY_TOLERANCE[14336])
ENTRY_EXACT = {8324: "d_flat_8192_of_8324", 14336: "e_wide_8192_of_14336"}
ENTRY_SEED, ENTRY_STEP = 0x00C0FFEE12345678, 2 ** 32 + 9


def entry_counters(B):
    """the entry-point test's counters: a call without records draws row b from stream b, so every form uses that"""
    return [(ENTRY_SEED, b) for b in range(B)], ENTRY_STEP


def case_id(case):
    V, scale, s = case
    return f"V{V}-{s}" + ("" if scale is None else f"-scale{scale:g}")


def tolerance_case(case):
    """(x float32 [V], p float64 [V], (temperature, top_k, top_p, settings)) of one tolerance case: a row robust() admits -- from
    draw_robust at the vocabulary's own scale, by the same rule at another -- and its float64 distribution."""
    V, scale, s = case
    temp, k, top_p, st = SETTINGS[s]
    k = min(k, V)
    index = TOLERANCE_CASES.index(case)
    rng = np.random.default_rng(9100 + index)
    if scale is None:
        x = tu.draw_robust(rng, 4, V, st, temperature=temp, top_k=k, top_p=top_p)[0]
    else:
        for _ in range(8):
            x = (rng.standard_normal((1, V)) * scale).astype(np.float32)
            if bool(tu.robust(torch.from_numpy(x), st, temperature=temp, top_k=k, top_p=top_p)[0]):
                break
        else:
            raise AssertionError(f"no robust row at V={V} scale={scale} {s}")
        x = x[0]
    return x, reference_probs(x, temp, k, top_p, st), (temp, k, top_p, st)


def reference_probs(x, temp, k, top_p, st=None):
    """float64 [V]: DecoderRef.masked_probs, or truncation_util.truncated_probs when truncation settings are on"""
    xt = torch.from_numpy(np.asarray(x, np.float32)).double()[None]
    if st:
        return tu.truncated_probs(xt, st, temp, k, top_p)[0][0].numpy()
    return DecoderRef.masked_probs(xt, temp, k if k else None, top_p)[0].numpy()
