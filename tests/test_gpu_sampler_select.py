"""The sampler's SELECTION (csrc/sampler.hip, the part of sample_kernel between the logit processors and the draw: top-k, then top-p)
on the MI355X against the host restatement of tests/sampler_select_util.py: the kept set, taken as `probs > 0` of the pre-draw
probabilities, against the integer tie rule (==) and the float64 nucleus band.  tests/test_sampler_select_host.py proves on the CPU that
every row of the case tables takes the code path its case names (pivot / candidates, both fallbacks, block-wide bisection, tie trim;
candidate list, mass histogram, its fallback, "everything"), and the input condition of the tolerance rows.

Every case is one launch of <= 16 rows, run under both values of sampler_wave_select: the two runs must be bit-equal, and each must
satisfy the host rule.  Rows that share their settings go through ops.sample, the others through ops.sample_rows.

* Exact rows (assertion == on the id set): top-k at temperatures 1, 0.5 and 2, whose division is exact, and at 0.7 on rows whose k-th
  and (k+1)-th quotients are more than 4 ulp apart; three-level rows whose nucleus at top_p 0.7 is the same set for top_p 0.7 +- 1e-3;
  rows of +0.0 and -0.0 entries (two keys, one exp) whose masses are exact and EQUAL top_p: a mass equal to top_p has reached it.
* Tolerance rows: check_nucleus() -- the kept set is a non-empty prefix of the descending order made of whole groups of equal logits
  (exact, whatever the arithmetic) and its length lies in nucleus_band(delta = 2e-5).  2e-5 is the project's fp32 row-operation bound,
  the one tests/test_gpu_sampler_draw.py derives for the same arithmetic; what it has to cover here, in units of the normalised mass
  the kernel compares with top_p:
      the total Z the masses are normalised by: at most 56 (registers) + 6 (lanes) + 4 (waves) = 66 fp32 additions, each rounding a
          value <= Z by at most 2^-24 of it                                                                      66 * 6e-8 = 4e-6
      x / temperature (half an ulp of |x| <= 32 in the exponent) and __expf: a relative 2e-6 on every term, at most twice that on
          a normalised partial sum                                                                                          4e-6
      the reciprocal 1 / Z and the one multiply per mass, half an ulp each                                                  1.2e-7
      the floor to the 2^-40 fixed point, one unit per entry: V * 2^-40 at V = 14336                                        1.3e-8
      the target floor(top_p * 2^40): 2^-40; the 64-bit integer sums (hi << 20) + lo: exact                                   1e-12
  together 8.2e-6 in the worst case, under the bound.  The host test shows that at this delta at least 75 % of every tolerance case's
  rows admit exactly ONE prefix length (most cases: all rows), so the assertion is close to an equality.
* Probabilities, every row: probs equals the float64 softmax over the device's own kept set (atol 2e-6, rtol 1e-4) and sums to 1
  within 1e-5; the drawn id is a kept one.

Observed on an MI355X, per case the largest delta any row NEEDS (0: its length is the float64 rule's own at delta 0), bound 2e-5:
    k_ties_p0.5_V{8324, 14336}, p_hist_V{40, 300, 8324, 9217, 14336}, p_behind_k_V{40, 300, 8324, 9217, 14336}, p_hist_scale12_V8324,
    p_hist_uniform_V{8324, 14336}, p_fallback_V{8324, 14336}, p_full_wave_V8324, per_row_V8324: 199 rows          0   (slack 2e-5)
    p_all_behind_k_V8324, 16 rows (top_p one ulp below 1)                                                          0
    p_all, 5 rows: 3 keep less than everything -- entries whose mass floors to 0 in the 2^-40 fixed point go      9.9e-8 (slack 1.99e-5)
    every entry point at V = 8324 and 14336, 2 x 16 x 8 tolerance rows                                             0
The exact rows have no distance: their id sets are equal.  Under planted in-bounds errors every case was seen
to fail."""
import numpy as np
import pytest
import torch

import sampler_select_util as S

pytestmark = pytest.mark.gpu
CASES = S.cases()
SEED, STEP = 0x5E1EC7000000D00D, 6


def launch(rows, seed=SEED, step=STEP):
    """one launch: (ids int64 [B], probs float32 [B, V]) on the host"""
    from mgea import ops
    from mgea.decoder import RowSampling
    dev = torch.from_numpy(np.stack([r["x"] for r in rows])).cuda()
    same = S.uniform(rows)
    if same is not None:
        T, k, p = same
        ids, probs = ops.sample(dev, T, k, p, seed=seed, step=step, want_probs=True)
    else:
        recs = [RowSampling(r["T"], r["k"], r["p"], seed=seed + b) for b, r in enumerate(rows)]
        ids, probs = ops.sample_rows(dev, recs, step=step, want_probs=True)
    return ids.cpu().numpy().astype(np.int64), probs.cpu().numpy()


def check_row(r, drawn, probs, what):
    """one row against its rule; returns the delta the row needs (0 for an exact row)"""
    x = S.scaled(r["x"], r["T"])
    got = probs > 0
    need = 0.0
    if r["kind"] == "band":
        n, n_lo, n_hi, need = S.check_nucleus(got, x, S.topk_kept(x, r["k"]), r["p"], S.DELTA, what)
    else:
        want = S.expected_exact(r)
        assert np.array_equal(got, want), (f"{what}: kept {int(got.sum())} ids, the rule keeps {int(want.sum())}; missing "
                                           f"{np.flatnonzero(want & ~got)[:8].tolist()}, extra {np.flatnonzero(got & ~want)[:8].tolist()}")
    p64 = S.softmax64(x, got)
    err = np.abs(probs.astype(np.float64) - p64)
    assert (err <= 2e-6 + 1e-4 * p64).all(), f"{what}: probabilities off the float64 softmax over the kept set by {float(err.max()):.3e}"
    assert abs(float(probs.astype(np.float64).sum()) - 1.0) <= 1e-5, f"{what}: probabilities sum to {float(probs.astype(np.float64).sum())!r}"
    drawn = np.atleast_1d(drawn)
    assert got[drawn].all(), f"{what}: drew {drawn[~got[drawn]][:4].tolist()}, not kept"
    return need


def report(name, needs):
    if needs:
        print(f"OBSERVED {name}: largest delta a row needs {max(needs):.3e}, smallest slack inside the band {S.DELTA - max(needs):.3e} "
              f"({sum(1 for v in needs if v > 0)} of {len(needs)} rows off the float64 length)")


# ------------------------------------------------------------------------------------------------------------- 1. the case tables
@pytest.mark.parametrize("name", list(CASES))
def test_selection_follows_the_rule(name, tune):
    rows = CASES[name]
    out = {}
    for sw in (1, 0):
        tune("sampler_wave_select", sw)
        out[sw] = launch(rows)
    needs = []
    for sw in (1, 0):
        ids, probs = out[sw]
        for b, r in enumerate(rows):
            tag = f"{name} row {b} (T {r['T']}, k {r['k']}, p {r['p']}; {r['kpath']} / {r['ppath']}; wave_select {sw})"
            need = check_row(r, ids[b], probs[b], tag)
            if r["kind"] == "band" and sw == 1:
                needs.append(need)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), f"{name}: sampler_wave_select 0 and 1 differ"
    report(name, needs)


# ------------------------------------------------------------------------------------------------------------- 2. cuts that are off
def test_cuts_that_are_off_change_nothing(tune):
    """top_p <= 0, top_p >= 1 and top_k >= V are "off": bit for bit the run without them"""
    from mgea import ops
    rows = CASES["k_fast_uniform_V8324"]
    V = len(rows[0]["x"])
    dev = torch.from_numpy(np.stack([r["x"] for r in rows])).cuda()

    def run(T, k, p):
        ids, probs = ops.sample(dev, T, k, p, seed=SEED, step=STEP, want_probs=True)
        return ids.cpu(), probs.cpu()

    for sw in (1, 0):
        tune("sampler_wave_select", sw)
        for T in (1.0, 0.7):
            for k, p in ((0, None), (50, None), (200, None), (0, 0.9)):
                base = run(T, k, p)
                if p is None:
                    assert int((base[1] > 0).sum(1).max()) == (k or V)
                variants = [(k, q) for q in (-0.5, 1.0, 1.5)] if p is None else []
                variants += [(V, p)] if k == 0 else []
                for k2, p2 in variants:
                    got = run(T, k2, p2)
                    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), f"T {T}: ({k2}, {p2}) against ({k}, {p}), wave_select {sw}"


# ------------------------------------------------------------------------------------------------------------- 3. every instantiation
@pytest.mark.parametrize("V", sorted(S.ENTRY_TIES))
def test_every_instantiation_selects_by_the_rule(V, monkeypatch):
    """one exact tie case and one tolerance case through every entry point of tests/test_gpu_sampler_draw.py's entry_points() -- one per
    <PENALTY, BIAS, ScoreArgs, GrammarArgs, TruncArgs> instantiation of sample_kernel at either register width, neutral settings.  The
    helper's calls do not ask for the pre-draw probabilities: every op it goes through is wrapped to ask for them and to hand back what
    the helper expects.  The scored forms' choice log-probability of the drawn id is finite: the id is in the expected set."""
    from mgea import ops
    from test_gpu_sampler_draw import B, entry_points
    seen = []

    def asking(fn):
        def call(*a, **kw):
            out = fn(*a, want_probs=True, **kw)
            seen.append(out[-1])
            return out[0] if len(out) == 2 else out[:-1]
        return call

    for op in ("sample", "sample_rows", "sample_rows_scored", "sample_rows_grammar", "sample_rows_truncated"):
        monkeypatch.setattr(ops, op, asking(getattr(ops, op)))
    n_scored, needs = 0, []
    for case in (S.ENTRY_TIES[V], S.ENTRY_BAND[V]):
        rows = CASES[case]
        T, k, p = S.uniform(rows)
        n = len(rows)
        assert B % n == 0 and len(rows[0]["x"]) == V
        dev = torch.from_numpy(np.stack([r["x"] for r in rows])).repeat(B // n, 1).cuda()       # row b is case row b % n, stream b
        for name, call in entry_points(V).items():
            del seen[:]
            ids, ch = call(dev, T, k, p, SEED, STEP)
            assert len(seen) == 1, f"{name}: {len(seen)} sampler ops ran"
            ids = ids.cpu().numpy().astype(np.int64)
            probs = seen[0]
            assert torch.equal(probs, probs[:n].repeat(B // n, 1)), f"V={V} {name}: equal rows, different probabilities"
            probs = probs[:n].cpu().numpy()
            for b, r in enumerate(rows):
                need = check_row(r, ids[b::n], probs[b], f"V={V} {name}: {case} row {b}")
                if r["kind"] == "band":
                    needs.append(need)
            if ch is not None:
                n_scored += 1
                assert bool(torch.isfinite(ch).all()), f"V={V} {name}: choice log-probability of a kept id is not finite"
    assert n_scored == 2 * 7
    report(f"entry points V={V}", needs)
