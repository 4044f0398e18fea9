"""The sampler's SELECTION restated on the host (tests/test_sampler_select_host.py proves its premises on the CPU,
tests/test_gpu_sampler_select.py holds csrc/sampler.hip to it on the MI355X): which ids top-k and top-p keep, written from the rule
in sampler.hip's header comment and include/mgea.h alone, and two predictors that say -- from integers and IEEE float32 arithmetic the
host reproduces exactly -- which of the kernel's code paths a row takes.

THE RULE.  x = logits / temperature, one float32 division per entry (scaled()).
    top-k   0 < k < V: keep every entry greater than the k-th largest, then the entries EQUAL to it by ascending id until exactly k are
            kept (topk_kept(); integers only: the order-preserving key of fkey()).  Otherwise the cut is off.
    top-p   0 < top_p < 1, over what top-k kept, by descending logit, equal logits forming one group that is kept or dropped whole:
            keep {logit >= boundary}, the boundary the largest logit at which the kept mass reaches top_p -- a group is kept iff the
            mass of the strictly larger logits is below top_p.  At least one id is kept.  Otherwise the cut is off.
The kernel decides the nucleus on fp32 masses floored to 2^-40, so a float64 restatement pins the LENGTH of the kept prefix to a band
(nucleus_band(), delta 2e-5: derived in tests/test_gpu_sampler_select.py) and everything else exactly (check_nucleus()): the kept set is
a prefix of the descending order, whole groups, never empty.

numpy / CPU torch only, no device code."""
import functools
import math

import numpy as np

DELTA = 2e-5            # the project's fp32 row-operation bound (tests/sampler_draw_util.py, DELTA)
UNIQUE_SHARE = 0.75     # the input condition: at least this share of a tolerance case's rows have n_lo == n_hi at DELTA
SAMP_NT, WAVE, SAMP_NW = 256, 64, 4     # thread t owns ids t + 256 j; wave w is threads 64 w .. 64 w + 63
KFAST = 64              # top_k <= 64 takes the pivot / candidate path, a wave holds at most 64 candidates
HSPAN = np.float32(28.0)
EDGE = 1e-3             # a nucleus path counts as forced when the boundary is this much mass away from its bucket's edges
NINF = -np.inf


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def fkey(x32):
    """The order-preserving uint32 key of a float32: a larger float has a larger key (-0.0 below +0.0)."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def scaled(x32, T):
    """x32 / float32(T) in float32 (IEEE: the build has no fast-math); T == 1 leaves the row as it is."""
    x32 = np.asarray(x32, np.float32)
    return x32 if float(T) == 1.0 else (x32 / np.float32(T)).astype(np.float32)


def topk_on(k, V):
    return k is not None and 0 < int(k) < V


def topp_on(top_p):
    return top_p is not None and 0.0 < float(np.float32(top_p)) < 1.0


def topk_kept(x32, k):
    """bool [V]: the exact kept set of top-k (everything when the cut is off)."""
    x32 = np.asarray(x32, np.float32)
    V = x32.shape[0]
    if not topk_on(k, V):
        return np.ones(V, bool)
    key = fkey(x32)
    kth = np.sort(key)[V - int(k)]
    keep = key > kth
    tied = np.flatnonzero(key == kth)                      # ascending ids
    keep[tied[:int(k) - int(keep.sum())]] = True
    return keep


def descending(x32, kept):
    """the kept ids by descending logit, equal logits by ascending id"""
    ids = np.flatnonzero(kept)
    return ids[np.lexsort((ids, -np.asarray(x32, np.float64)[ids]))]


def _groups(x64, order):
    """(ends, excl, incl): for every group of equal logits along `order` the prefix length at its end, the float64 mass of the strictly
    larger logits and the mass down to and including the group"""
    v = x64[order]
    p = np.exp(v - v[0])
    p = p / p.sum()
    ends = np.flatnonzero(np.append(v[1:] != v[:-1], True)) + 1
    incl = np.cumsum(p)[ends - 1]
    incl[-1] = 1.0
    excl = np.concatenate([[0.0], incl[:-1]])
    return ends, excl, incl


def nucleus_band(x64, kept, top_p, delta):
    """(n_lo, n_hi): the admissible lengths of the kept prefix of descending(x64, kept).  A prefix that ends with a group is admissible
    iff the mass strictly above that group is < top_p + delta and the mass including it is >= top_p - delta."""
    x64 = np.asarray(x64, np.float64)
    ends, excl, incl = _groups(x64, descending(x64, kept))
    ok = np.flatnonzero((excl < top_p + delta) & (incl >= top_p - delta))
    return int(ends[ok[0]]), int(ends[ok[-1]])


def check_nucleus(got_kept, x32, kept, top_p, delta, what=""):
    """The assertion: got_kept (bool [V]) is a non-empty prefix of descending(x32, kept) made of whole groups, and its length lies in
    nucleus_band().  Returns (n, n_lo, n_hi, need): need = the delta at which the length would just be admitted (0: admissible at
    delta = 0), so delta - need is the slack by which the prefix sits inside its band."""
    x32 = np.asarray(x32, np.float32)
    top_p = float(np.float32(top_p))
    got = np.flatnonzero(got_kept)
    n = len(got)
    assert n >= 1, f"{what}: nothing kept"
    order = descending(x32, kept)
    assert n <= len(order) and np.array_equal(np.sort(order[:n]), got), \
        (f"{what}: the {n} kept ids are not the first {n} of the descending order; missing {np.setdiff1d(order[:n], got)[:8].tolist()}, "
         f"extra {np.setdiff1d(got, order[:n])[:8].tolist()}")
    assert n == len(order) or x32[order[n - 1]] > x32[order[n]], f"{what}: the kept prefix of {n} cuts a group of equal logits"
    x64 = x32.astype(np.float64)
    ends, excl, incl = _groups(x64, order)
    g = int(np.searchsorted(ends, n))
    need = max(excl[g] - top_p, top_p - incl[g], 0.0)
    n_lo, n_hi = nucleus_band(x64, kept, top_p, delta)
    assert n_lo <= n <= n_hi, (f"{what}: kept {n}, admissible [{n_lo}, {n_hi}] at top_p {top_p!r} delta {delta}: mass above the last group "
                               f"{excl[g]!r}, with it {incl[g]!r} (needs delta {need:.3e})")
    return n, n_lo, n_hi, need


# ---- the path predictors ------------------------------------------------------------------------------------------------------------
def _registers(a, fill):
    """[V] -> [registers, 256]: column t is thread t's entries"""
    V = a.shape[0]
    out = np.full(-(-V // SAMP_NT) * SAMP_NT, fill, a.dtype)
    out[:V] = a
    return out.reshape(-1, SAMP_NT)


def topk_path(x32, k):
    """'off', 'fast', 'fast_ties', 'fallback_pivot0', 'fallback_overflow' (top_k <= 64) or 'block', 'block_ties' (top_k > 64), from the
    integer pivot rule alone: every wave takes the ceil(k / 4)-th largest of its 64 lane maxima (0 with fewer valid lanes), the pivot is
    the smallest of the four, and a wave with more than 64 keys >= pivot overflows its candidate slots."""
    x32 = np.asarray(x32, np.float32)
    V, k = x32.shape[0], int(k or 0)
    if not topk_on(k, V):
        return "off"
    key = fkey(x32)
    ties = int((key >= np.sort(key)[V - k]).sum()) > k
    if k > KFAST:
        return "block_ties" if ties else "block"
    K = _registers(key, np.uint32(0))
    lane_max = K.max(0)
    j = -(-k // SAMP_NW)
    pivot = None
    for w in range(SAMP_NW):
        lm = np.sort(lane_max[WAVE * w:WAVE * (w + 1)])[::-1]
        p = int(lm[j - 1])          # 0 = an invalid lane: fewer than j lanes of the wave own an id
        pivot = p if pivot is None else min(pivot, p)
    if pivot == 0:
        return "fallback_pivot0"
    if max(int((K[:, WAVE * w:WAVE * (w + 1)] >= pivot).sum()) for w in range(SAMP_NW)) > KFAST:
        return "fallback_overflow"
    return "fast_ties" if ties else "fast"


def buckets(x32, kept):
    """int [V]: the mass histogram's bucket of every entry, float32 as on the device: scale = 255.99f / (mx - lowest), lowest the
    smallest kept logit within 28 units of the maximum; bucket = int((mx - x) * scale), 255 beyond."""
    x32 = np.asarray(x32, np.float32)
    key = fkey(x32)                          # (the extremes by key: +0.0 lies above -0.0)
    mx = x32[kept][np.argmax(key[kept])]
    span = kept & (x32 >= mx - HSPAN)
    lowest = x32[span][np.argmin(key[span])]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = ((mx - x32) * (np.float32(255.99) / (mx - lowest))).astype(np.float32)
    return np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=255.0).clip(max=255.0).astype(np.int64)     # NaN (0 * inf) -> 0; +inf and beyond -> 255


def nucleus_path(x32, kept, top_p, cover=False):
    """(path, info): 'candidates' (cover: top-k took the fast path and met no ties, so its candidate list holds the kept set), 'all'
    (top_p within DELTA of 1: whether the floored masses reach the target is below the arithmetic's resolution), 'hist_wave' or
    'hist_fallback' (the boundary bucket puts more than 64 entries into one wave).  info: the boundary bucket, the largest per-wave
    population of it and of its two neighbours, the mass between the boundary and the nearer bucket edge, and `forced`: all three
    buckets give the same verdict, or that mass is at least EDGE."""
    top_p = float(np.float32(top_p))
    if top_p >= 1.0 - DELTA:
        return "all", dict(forced=True)
    if cover:
        return "candidates", dict(forced=True)
    x32 = np.asarray(x32, np.float32)
    V = x32.shape[0]
    x64 = x32.astype(np.float64)
    p = np.where(kept, np.exp(x64 - x64[kept].max()), 0.0)
    p /= p.sum()
    live = kept & (p * 2.0 ** 40 >= 1.0)      # entries whose fixed-point mass is not 0
    b = buckets(x32, kept)
    cum = np.cumsum(np.bincount(b[live], weights=p[live], minlength=256))
    bstar = int(min(np.searchsorted(cum, top_p), 255))
    wave = (np.arange(V) % SAMP_NT) // WAVE

    def pop(bk):
        if not 0 <= bk <= 255:
            return None
        return max(int((live & (b == bk) & (wave == w)).sum()) for w in range(SAMP_NW))

    pops = [pop(bstar - 1), pop(bstar), pop(bstar + 1)]
    edge = min(top_p - (cum[bstar - 1] if bstar else 0.0), cum[bstar] - top_p)
    verdicts = {q > KFAST for q in pops if q is not None}
    return ("hist_fallback" if pops[1] > KFAST else "hist_wave"), dict(bucket=bstar, pops=pops, edge=float(edge),
                                                                      forced=len(verdicts) == 1 or edge >= EDGE)


def row_paths(row):
    """(top-k path, nucleus path or None, info) of a case row"""
    x = scaled(row["x"], row["T"])
    kp = topk_path(x, row["k"])
    if not topp_on(row["p"]):
        return kp, None, {}
    pp, info = nucleus_path(x, topk_kept(x, row["k"]), row["p"], cover=kp == "fast")
    return kp, pp, info


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _rng(*tag):
    return np.random.default_rng([9300] + [int(t) for t in tag])


def randn_row(tag, V, scale):
    return (_rng(*tag).standard_normal(V) * scale).astype(np.float32)


def row(x, T=1.0, k=0, p=None, kpath=None, ppath=None, kind="exact_k", **extra):
    """kind: 'exact_k' (the kept set is topk_kept, ==), 'exact_p' (it is extra['expect'], ==), 'band' (check_nucleus)"""
    return dict(x=np.asarray(x, np.float32), T=float(T), k=int(k), p=p, kpath=kpath, ppath=ppath, kind=kind, **extra)


def tie_row(tag, V, group, need, k):
    """A row whose k-th largest value is shared by the ids `group`: k - need distinct larger entries elsewhere, a background far below,
    so top-k keeps the `need` lowest ids of the group.  Returns (x, the tied ids kept)."""
    rng = _rng(*tag)
    group = np.sort(np.asarray(group, np.int64))
    x = (rng.standard_normal(V) - 6.0).astype(np.float32).clip(max=-2.0)
    rest = np.setdiff1d(np.arange(V), group)
    above = rng.choice(rest, k - need, replace=False)
    x[above] = (1.0 + 2.0 * rng.random(k - need)).astype(np.float32)
    x[group] = 0.5
    assert len(np.unique(x[above])) == len(above) and 0 < need <= len(group)
    return x, group[:need]


def tie_layouts(V):
    """name -> (tied ids, need): where the cut between kept and trimmed ties falls"""
    last = -(-V // SAMP_NT) - 1                     # the last register, partly valid unless 256 divides V
    r = 3 * SAMP_NT
    return {
        "inside_a_wave": (r + 64 + np.arange(5, 26), 10),                     # lanes 5..25 of wave 1, register 3: the cut between lanes 14 | 15
        "at_a_wave_boundary": (r + np.arange(40, 90), 24),                    # ids r + 40 .. r + 63 kept: wave 0's last lane | wave 1's first
        "at_a_register_boundary": (4 * SAMP_NT + np.arange(-20, 20), 20),     # ids 256 j - 20 .. 256 j - 1 kept
        "last_register": (np.arange(V - 24, V), 22),                          # V = 8324: ids 8300 .. 8323 of register 32, waves 1 | 2
        "scattered": (np.arange(11, V, 97)[:40], 17),
        "one_wave_100": ((np.arange(10)[:, None] * SAMP_NT + np.arange(10)[None]).reshape(-1), 37),     # 100 ties in wave 0
        "first_register_id_0": (np.arange(0, 30), 1),
    }, last


def three_level(tag, V, group, tail_shift=-12.0):
    """One entry at 0 (id 845 % V), `group` tied at log(0.7 / g) -- 0.7 of the top entry's mass in total, ~0.4 of the row's -- and a tail
    of randn * 0.3 + tail_shift carrying ~0.03: at top_p 0.7 the top entry alone (0.57) falls short and the group (0.97 with it) must
    be kept whole."""
    rng = _rng(*tag)
    group = np.asarray(group, np.int64)
    x = (rng.standard_normal(V) * 0.3 + tail_shift).astype(np.float32)
    x[group] = np.float32(math.log(0.7 / len(group)))
    top = 845 % V
    assert top not in group
    x[top] = 0.0
    return x, top


def fallback_row(tag, V, n=400):
    """randn * 0.3 - 12 background, one entry at 0, one at -20 (it widens the histogram's span), n entries -3 + U(0, 0.03) at wave-0 ids:
    the nucleus boundary of top_p 0.55 .. 0.8 lies among the n, which share a few buckets and one wave"""
    rng = _rng(*tag)
    x = (rng.standard_normal(V) * 0.3 - 12.0).astype(np.float32)
    wave0 = np.flatnonzero((np.arange(V) % SAMP_NT) < WAVE)
    ids = rng.choice(wave0[(wave0 != 5) & (wave0 != 6)], n, replace=False)
    x[ids] = (-3.0 + 0.03 * rng.random(n)).astype(np.float32)
    x[5], x[6] = 0.0, -20.0
    return x


T_EXACT = (1.0, 0.5, 2.0)       # the division by these is exact
T_TOL = (1.0, 0.7, 1.3)
VOCABS = (40, 300, 8324, 9217, 14336)


def _ulp_gap_ok(x32, T, k, ulps=4):
    """the k-th and (k+1)-th largest quotients differ by more than `ulps` ulp: a division off by an ulp could not reorder them"""
    s = np.sort(fkey(scaled(x32, T)).astype(np.int64))[::-1]
    return int(s[k - 1] - s[k]) > ulps


@functools.lru_cache(maxsize=None)
def cases():
    """name -> list of rows (<= 16, one launch); rows that share (T, k, p) run through ops.sample, the others through ops.sample_rows"""
    c = {}
    # -- top-k, exact.  Random rows: the pivot / candidate path
    for V in (300, 8324, 9217, 14336):
        c[f"k_fast_V{V}"] = [row(randn_row((1, V, i), V, 3.0), T, k, kpath="fast")
                              for i, (k, T) in enumerate((k, T) for k in (2, 7, 50, 63, 64) for T in T_EXACT)]
    c["k_fast_uniform_V8324"] = [row(randn_row((2, i), 8324, 3.0), 1.0, 50, kpath="fast") for i in range(8)]
    c["k_pivot0_V40"] = [row(randn_row((3, i), 40, 3.0), T, k, kpath="fallback_pivot0") for i, (k, T) in
                         enumerate((k, T) for k in (2, 7) for T in T_EXACT)]
    c["k_pivot0_V200_k64"] = [row(randn_row((4, i), 200, 3.0), 1.0, 64, kpath="fallback_pivot0") for i in range(6)]   # wave 3: 8 valid lanes
    rows = []
    for i, k in enumerate((8, 50, 8, 50, 8, 50)):
        x = (-2.0 + 0.01 * _rng(5, i).standard_normal(8324)).astype(np.float32)
        wave0 = np.flatnonzero((np.arange(8324) % SAMP_NT) < WAVE)
        ids = _rng(5, i, 1).choice(wave0, 200, replace=False)
        x[ids] = (1.0 + 0.02 * _rng(5, i, 2).permutation(200)).astype(np.float32)       # 200 large distinct entries, wave 0 only
        rows.append(row(x, T_EXACT[i % 3], k, kpath="fallback_overflow"))
    c["k_overflow_V8324"] = rows
    # a wave whose candidate slots are exactly full: the 64 largest entries in wave 0's 64 lanes, 16 smaller ones in 16 lanes of each
    # other wave, so the pivot is the smallest of those 48 and wave 0 publishes 64 keys -- slot 63 holds the 64-th largest of the row
    rows = []
    for i, T in enumerate(T_EXACT):
        rng = _rng(19, i)
        x = (rng.standard_normal(8324) - 8.0).astype(np.float32).clip(max=-4.0)
        regs = rng.integers(0, 32, SAMP_NT)
        big = np.arange(WAVE) + SAMP_NT * regs[:WAVE]
        x[big] = (4.0 + rng.permutation(WAVE) / 16.0).astype(np.float32)
        last, least = big.max(), big[np.argmin(x[big])]      # the highest id is the wave's 64-th candidate: it gets the 64-th largest value
        x[last], x[least] = x[least], x[last]
        for w in (1, 2, 3):
            lanes = WAVE * w + rng.choice(WAVE, 16, replace=False)
            x[lanes + SAMP_NT * regs[lanes]] = (1.0 + rng.permutation(16) / 16.0).astype(np.float32)
        x[lanes[0] + SAMP_NT * regs[lanes[0]]] = np.nextafter(x[last], np.float32(NINF))     # the 65-th largest: one ulp below the 64-th
        rows.append(row(x, T, 64, kpath="fast"))
    c["k_fast_full_wave_V8324"] = rows
    for V in (8324, 14336):
        c[f"k_block_V{V}"] = [row(randn_row((6, V, i), V, 3.0), T, k, kpath="block")
                               for i, (k, T) in enumerate((k, T) for k in (65, 200, 1000, V - 1) for T in T_EXACT)]
    # -- ties: the cut of the trim in every place, under the candidate path (k = 50) and the block-wide one (k = 200); then the same
    # rows with top_p 0.5 behind them (the survivors go through the mass histogram: the candidate list does not cover them)
    for V in (8324, 14336):
        layouts, _ = tie_layouts(V)
        rows = []
        for i, (name, (group, need)) in enumerate(layouts.items()):
            for k in (50, 200):
                x, kept_ties = tie_row((7, V, i, k), V, group, need, k)
                kpath = "block_ties" if k > KFAST else "fallback_overflow" if name == "one_wave_100" else "fast_ties"
                rows.append(row(x, 1.0, k, kpath=kpath, layout=name, kept_ties=kept_ties, group=np.asarray(group)))
        c[f"k_ties_V{V}"] = rows
        c[f"k_ties_p0.5_V{V}"] = [dict(r, p=0.5, kind="band", ppath="hist_wave") for r in rows]
        c[f"k_ties_uniform_V{V}"] = [r for r in rows if r["k"] == 50] + [row(np.full(V, 1.25, np.float32), 1.0, 50, kpath="fallback_overflow")]
    c["k_all_equal_V8324"] = [row(np.full(8324, v, np.float32), 1.0, k, kpath=kp) for v, k, kp in
                              ((1.25, 64, "fallback_overflow"), (-3.0, 200, "block_ties"))]
    c["k_all_equal_V14336"] = [row(np.full(14336, v, np.float32), 1.0, k, kpath=kp) for v, k, kp in
                               ((0.0, 7, "fallback_overflow"), (2.5, 65, "block_ties"), (-0.0, 14335, "block_ties"))]
    # -- rows with -inf entries: fewer finite entries than k, so -inf entries sit among the kept and carry probability exactly 0
    rows = []
    for i, (n_fin, k) in enumerate(((30, 50), (1, 7), (63, 64), (100, 200), (150, 1000))):
        x = np.full(8324, NINF, np.float32)
        ids = _rng(8, i).choice(8324, n_fin, replace=False)
        x[ids] = randn_row((8, i, 1), n_fin, 3.0)
        rows.append(row(x, T_EXACT[i % 3], k, kpath="block_ties" if k > KFAST else "fallback_overflow", finite=np.sort(ids)))
    c["k_minus_inf_V8324"] = rows
    # -- T = 0.7: rows whose k-th and (k+1)-th quotients differ by more than 4 ulp
    rows = []
    for i in range(40):
        k = (2, 7, 50, 64, 65, 200)[i % 6]
        x = randn_row((9, i), 8324, 3.0)
        if _ulp_gap_ok(x, 0.7, k) and len(rows) < 12:
            rows.append(row(x, 0.7, k, kpath="block" if k > KFAST else "fast"))
    c["k_T0.7_V8324"] = rows

    # -- top-p, exact: three-level rows at top_p 0.7
    for V in (8324, 14336):
        rows = []
        g8 = np.asarray([3, 70, 130, 200, 256 + 9, 5 * 256 + 100, 20 * 256 + 250, V - 2])       # over waves and registers
        x, top = three_level((10, V, 0), V, g8)
        rows.append(row(x, 1.0, 0, 0.7, ppath="hist_wave", kind="exact_p", expect=np.sort(np.append(g8, top))))
        g300 = (np.arange(5)[:, None] * SAMP_NT + np.arange(60)[None]).reshape(-1)              # 300 ids of wave 0's lanes
        x, top = three_level((10, V, 1), V, g300)
        rows.append(row(x, 1.0, 0, 0.7, ppath="hist_fallback", kind="exact_p", expect=np.sort(np.append(g300, top))))
        x, top = three_level((10, V, 2), V, g8)
        rows.append(row(x, 1.0, 16, 0.7, kpath="fast", ppath="candidates", kind="exact_p", expect=np.sort(np.append(g8, top))))
        x, top = three_level((10, V, 3), V, g8)     # top_k 7 = the top entry and the six lowest ids of the group: 0.656 + 0.344
        rows.append(row(x, 1.0, 7, 0.7, kpath="fast_ties", ppath="hist_wave", kind="exact_p", expect=np.sort(np.append(g8[:6], top))))
        x, top = three_level((10, V, 4), V, g300)
        rows.append(row(x, 1.0, 201, 0.7, kpath="block_ties", ppath="hist_fallback", kind="exact_p", expect=np.sort(np.append(g300[:200], top))))
        c[f"p_exact_V{V}"] = rows

    # -- top-p, tolerance.  Per vocabulary: the histogram alone, behind a candidate top-k, behind a block-wide one
    for V in VOCABS:
        rows, i = [], 0
        for scale in (3.0, 6.0):
            for p in (0.3, 0.9):
                for T in T_TOL:
                    rows.append(row(randn_row((11, V, i), V, scale), T, 0, p, ppath="hist_wave", kind="band"))
                    i += 1
        c[f"p_hist_V{V}"] = rows
        rows, i = [], 0
        for scale in (3.0, 6.0):
            for k in (7, 50, 64, 65, 200):
                if k >= V:
                    continue
                for p in (0.3, 0.9) if k in (7, 50, 200) else (0.9,):
                    T = T_TOL[i % 3]
                    # (V = 40: three waves own no id, the pivot is 0 and the candidate list is never made)
                    kp = "block" if k > KFAST else "fast" if V >= SAMP_NT else "fallback_pivot0"
                    rows.append(row(randn_row((12, V, i), V, scale), T, k, p, kpath=kp, ppath="candidates" if kp == "fast" else "hist_wave",
                                    kind="band"))
                    i += 1
        c[f"p_behind_k_V{V}"] = rows
    c["p_hist_scale12_V8324"] = [row(randn_row((13, i), 8324, 12.0), T, 0, p, ppath="hist_wave", kind="band")
                                 for i, (p, T) in enumerate((p, T) for p in (0.3, 0.9, 0.999) for T in T_TOL)]
    c["p_hist_uniform_V8324"] = [row(randn_row((14, i), 8324, 3.0 if i % 2 else 6.0), 0.7, 0, 0.9, ppath="hist_wave", kind="band") for i in range(8)]
    c["p_hist_uniform_V14336"] = [row(randn_row((15, i), 14336, 3.0 if i % 2 else 6.0), 1.3, 0, 0.3, ppath="hist_wave", kind="band") for i in range(8)]
    for V in (8324, 14336):
        c[f"p_fallback_V{V}"] = [row(fallback_row((16, V, i), V), 1.0, 0, p, ppath="hist_fallback", kind="band")
                                 for i, p in enumerate((0.55, 0.7, 0.8))]
    # the boundary bucket holds exactly 64 entries of one wave (its candidate slots are full), the last of them -- the highest id --
    # the largest of the 64, always above the boundary
    rows = []
    for i, p in enumerate((0.55, 0.7, 0.8)):
        x = fallback_row((20, i), 8324, 64)
        ids = np.flatnonzero((x > -3.5) & (x < -2.5))
        x[ids[-1]] = -2.9695
        rows.append(row(x, 1.0, 0, p, ppath="hist_wave", kind="band", full_wave=ids))
    c["p_full_wave_V8324"] = rows
    # the mass on the edge: n ids at +0.0, m at -0.0 (the smaller key, the same exp), everything else -inf, n + m a power of two.  Every
    # mass is exact, n / (n + m) IS top_p, so the ids at +0.0 reach it and the others go: `>=` against `>` at the boundary
    rows = []
    for i, (n, m, p, wave0) in enumerate(((64, 64, 0.5, False), (1, 3, 0.25, False), (128, 128, 0.5, True), (8, 24, 0.25, False), (96, 32, 0.75, True))):
        rng = _rng(21, i)
        pool = np.flatnonzero((np.arange(8324) % SAMP_NT) < WAVE) if wave0 else np.arange(8324)
        ids = rng.choice(pool, n + m, replace=False)
        x = np.full(8324, NINF, np.float32)
        x[ids[:n]], x[ids[n:]] = 0.0, -0.0
        rows.append(row(x, 1.0, 0, p, ppath="hist_fallback" if wave0 else "hist_wave", kind="exact_p", expect=np.sort(ids[:n])))
    c["p_on_the_edge_V8324"] = rows
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    c["p_all"] = [row(randn_row((17, i), 8324, scale), T, k, p, kpath="fast" if k else None, ppath="all", kind="band")
                  for i, (scale, T, k, p) in enumerate(((3.0, 1.0, 0, 0.9999999), (3.0, 1.0, 0, below_one), (6.0, 0.7, 0, below_one),
                                                        (3.0, 1.3, 50, below_one), (6.0, 1.0, 50, 0.9999999)))]
    # ... and behind a candidate top-k, where "even everything weighs less than the target" must fall back to top-k's own boundary
    c["p_all_behind_k_V8324"] = [row(randn_row((22, i), 8324, 3.0 if i % 2 else 6.0), T_TOL[i % 3], (7, 50, 64, 33)[i % 4], below_one,
                                     kpath="fast", ppath="all", kind="band") for i in range(16)]
    # -- one launch in which every row has other settings
    specs = ((1.0, 50, 0.9), (0.7, 0, 0.3), (1.3, 7, None), (0.5, 200, None), (2.0, 64, 0.9), (1.0, 0, 0.9), (0.7, 65, 0.3), (1.3, 2, 0.9),
             (1.0, 1000, 0.9), (0.5, 63, None), (0.7, 0, 0.9), (1.3, 200, 0.3), (1.0, 0, None), (2.0, 8323, None))
    rows = []
    for i, (T, k, p) in enumerate(specs):
        kp = None if not k else "fast" if k <= KFAST else "block"
        pp = None if p is None else "candidates" if kp == "fast" else "hist_wave"
        rows.append(row(randn_row((18, i), 8324, 3.0 if i % 2 else 6.0), T, k, p, kpath=kp, ppath=pp, kind="band" if p else "exact_k"))
    c["per_row_V8324"] = rows
    for name, rows in c.items():
        assert 1 <= len(rows) <= 16 and len({len(r["x"]) for r in rows}) == 1, name
    return c


def uniform(rows):
    """(T, k, p) when every row of the case has the same settings (the case runs through ops.sample), else None"""
    s = {(r["T"], r["k"], r["p"]) for r in rows}
    return next(iter(s)) if len(s) == 1 else None


# the cases every entry point of the sampler is run on: one exact tie case and one tolerance case per kernel width, uniform settings
ENTRY_TIES = {8324: "k_ties_uniform_V8324", 14336: "k_ties_uniform_V14336"}
ENTRY_BAND = {8324: "p_hist_uniform_V8324", 14336: "p_hist_uniform_V14336"}


def expected_exact(r):
    """bool [V]: the ids an exact row keeps WITH MASS (top-k may also keep -inf entries: they carry probability 0)"""
    x = scaled(r["x"], r["T"])
    if r["kind"] == "exact_p":
        keep = np.zeros(len(x), bool)
        keep[r["expect"]] = True
        return keep
    return topk_kept(x, r["k"]) & np.isfinite(x)


def softmax64(x32, keep):
    x64 = np.asarray(x32, np.float64)
    p = np.where(keep, np.exp(x64 - x64[keep].max()), 0.0)
    return p / p.sum()
