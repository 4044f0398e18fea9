"""The premises of tests/sampler_select_util.py, on the CPU: the tie rule against torch.topk and hand-made rows, the nucleus band at
delta 0 against the oracle's float64 masked_probs, the path every case row claims (under the host predictors, with their margin), the
input condition of the tolerance cases (at least 75 % of a case's rows admit ONE prefix length at delta 2e-5) and the exact families'
independence of top_p +- 1e-3.  Conditions on the inputs and on the restatement, not on the code under test."""
import numpy as np
import pytest
import torch

import sampler_select_util as S
from oracle.decoder_ref import DecoderRef

CASES = S.cases()


def ids_of(mask):
    return np.flatnonzero(mask).tolist()


# ---------------------------------------------------------------------------------------------------------------- keys and ties
def test_fkey_preserves_the_order_of_floats():
    x = np.asarray([-np.inf, -3e38, -1.5, -1e-40, -0.0, 0.0, 1e-40, 2.0 ** -126, 1.0, 1.0000001, 3e38, np.inf], np.float32)
    key = S.fkey(x).astype(np.int64)
    assert (np.diff(key) > 0).all() and key.min() > 0          # 0 stays free for "not a candidate"
    r = (np.random.default_rng(1).standard_normal(4096) * 5).astype(np.float32)
    assert np.array_equal(np.argsort(S.fkey(r), kind="stable"), np.argsort(r, kind="stable"))
    assert np.array_equal(S.scaled(r, 0.5), r * np.float32(2)) and S.scaled(r, 1.0) is r
    assert np.array_equal(S.scaled(r, 0.7), (torch.from_numpy(r) / 0.7).numpy())


@pytest.mark.parametrize("V", [40, 300, 8324, 14336])
def test_topk_kept_is_torch_topk_without_ties(V):
    rng = np.random.default_rng(V)
    for k in (1, 2, 7, 50, 64, 65, 200, V - 1):
        if k >= V:
            continue
        x = (rng.standard_normal(V) * 3).astype(np.float32)
        s = np.sort(x)[::-1]
        assert s[k - 1] > s[k]                                     # no tie at the cut: torch.topk has one answer
        want = np.sort(torch.from_numpy(x).topk(k).indices.numpy())
        assert np.array_equal(np.flatnonzero(S.topk_kept(x, k)), want)
    for k in (0, None, V, V + 5):
        assert S.topk_kept(x, k).all()


def test_topk_kept_on_hand_made_ties():
    x = np.asarray([1, 3, 2, 3, 3, 0, 3], np.float32)
    assert ids_of(S.topk_kept(x, 1)) == [1]
    assert ids_of(S.topk_kept(x, 2)) == [1, 3]
    assert ids_of(S.topk_kept(x, 3)) == [1, 3, 4]
    assert ids_of(S.topk_kept(x, 4)) == [1, 3, 4, 6]
    assert ids_of(S.topk_kept(x, 5)) == [1, 2, 3, 4, 6]
    y = np.asarray([5, 2, 7, 2, 2, 9, 2], np.float32)             # larger entries first, then ties by ascending id
    assert ids_of(S.topk_kept(y, 4)) == [0, 1, 2, 5]
    assert ids_of(S.topk_kept(y, 5)) == [0, 1, 2, 3, 5]
    z = np.asarray([-np.inf, 1, -np.inf, -np.inf], np.float32)    # -inf is an ordinary value: lowest ids first
    assert ids_of(S.topk_kept(z, 3)) == [0, 1, 2]
    assert ids_of(S.topk_kept(np.asarray([0.0, -0.0, 0.0], np.float32), 2)) == [0, 2]      # -0.0 has the smaller key


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("k_ties_V")])
def test_tie_rows_keep_what_their_construction_says(name):
    for r in CASES[name]:
        keep = S.topk_kept(r["x"], r["k"])
        assert int(keep.sum()) == r["k"]
        assert np.array_equal(np.flatnonzero(keep[r["group"]]), np.arange(len(r["kept_ties"]))), r["layout"]
        assert np.array_equal(np.sort(r["group"])[:len(r["kept_ties"])], r["kept_ties"])
        assert 0 < len(r["kept_ties"]) < len(r["group"]) and keep[r["x"] > 0.5].all() and not keep[r["x"] < 0.5].any()


# ---------------------------------------------------------------------------------------------------------------- the band
@pytest.mark.parametrize("V", [40, 300, 8324])
def test_band_at_delta_0_is_the_oracles_kept_count(V):
    rng = np.random.default_rng(100 + V)
    for scale in (3.0, 6.0):
        for T in (1.0, 0.7, 1.3):
            for k in (0, 7, 50, 200):
                for top_p in (0.3, 0.9):
                    x = S.scaled((rng.standard_normal(V) * scale).astype(np.float32), T)
                    k_ = k if k < V else 0
                    x64 = torch.from_numpy(x).double()[None]
                    want = int((DecoderRef.masked_probs(x64, 1.0, k_ or None, top_p)[0] > 0).sum())
                    assert S.nucleus_band(x.astype(np.float64), S.topk_kept(x, k_), top_p, 0.0) == (want, want)


def test_band_on_hand_made_groups():
    # masses 0.4 | 0.2 0.2 (one group) | 0.1 | 0.1
    x = np.log(np.asarray([0.1, 0.2, 0.4, 0.2, 0.1])).astype(np.float32)
    x[3] = x[1]
    x[4] = np.nextafter(x[0], np.float32(-1e9))
    kept = np.ones(5, bool)
    assert S.nucleus_band(x, kept, 0.3, 0.0) == (1, 1)
    assert S.nucleus_band(x, kept, 0.5, 0.0) == (3, 3)            # the group of two is kept whole
    assert S.nucleus_band(x, kept, 0.85, 0.0) == (4, 4)
    assert S.nucleus_band(x, kept, 0.4, 1e-3) == (1, 3)           # top_p on the edge of the first entry: either side is admissible
    got = np.zeros(5, bool)
    got[[2, 1, 3]] = True
    assert S.check_nucleus(got, x, kept, 0.5, S.DELTA)[:3] == (3, 3, 3)
    for wrong, why in (([2, 1], "cuts a group"), ([2, 3, 0], "not the first"), ([2], "admissible"), ([2, 1, 3, 0], "admissible"), ([], "nothing")):
        bad = np.zeros(5, bool)
        bad[wrong] = True
        with pytest.raises(AssertionError, match=why):
            S.check_nucleus(bad, x, kept, 0.5, S.DELTA)


# ---------------------------------------------------------------------------------------------------------------- the paths
@pytest.mark.parametrize("name", list(CASES))
def test_every_row_takes_the_path_it_claims(name):
    for i, r in enumerate(CASES[name]):
        kp, pp, info = S.row_paths(r)
        assert kp == (r["kpath"] or "off"), f"{name} row {i}: top-k path {kp}, claimed {r['kpath']}"
        assert pp == r["ppath"], f"{name} row {i}: nucleus path {pp}, claimed {r['ppath']} ({info})"
        assert info.get("forced", True), f"{name} row {i}: {pp} is not forced: {info}"
        if r["T"] == 0.7 and r["kind"] == "exact_k":
            assert S._ulp_gap_ok(r["x"], r["T"], r["k"])


def test_the_tables_hold_every_path():
    seen_k, seen_p = set(), set()
    for rows in CASES.values():
        for r in rows:
            seen_k.add(r["kpath"])
            seen_p.add((r["ppath"], S.row_paths(r)[0]))
    assert seen_k >= {"fast", "fast_ties", "fallback_pivot0", "fallback_overflow", "block", "block_ties", None}
    assert {p for p, _ in seen_p} >= {"candidates", "hist_wave", "hist_fallback", "all", None}
    # the histogram behind every way top-k can end without covering the kept set
    assert {k for p, k in seen_p if p == "hist_wave"} >= {"off", "fast_ties", "fallback_overflow", "fallback_pivot0", "block", "block_ties"}
    layouts = {r["layout"] for r in CASES["k_ties_V8324"]}
    assert layouts >= {"inside_a_wave", "at_a_wave_boundary", "at_a_register_boundary", "last_register", "one_wave_100"}


# ---------------------------------------------------------------------------------------------------------------- the input condition
@pytest.mark.parametrize("name", [n for n, rows in CASES.items() if any(r["kind"] == "band" for r in rows)])
def test_tolerance_cases_admit_one_length_on_most_rows(name):
    """at delta 2e-5 at least 75 % of the case's rows have n_lo == n_hi.  The `all` rows are outside the condition by construction:
    top_p + delta > 1 admits every length from n_lo up, they assert the band's lower end and the exact properties alone."""
    one = []
    for r in CASES[name]:
        if r["kind"] != "band" or r["ppath"] == "all":
            continue
        x = S.scaled(r["x"], r["T"])
        n_lo, n_hi = S.nucleus_band(x.astype(np.float64), S.topk_kept(x, r["k"]), float(np.float32(r["p"])), S.DELTA)
        one.append(n_lo == n_hi)
    if not one:
        assert all(r["ppath"] == "all" for r in CASES[name])
        return
    share = float(np.mean(one))
    print(f"OBSERVED {name}: {share:.3f} of {len(one)} rows admit one prefix length at delta {S.DELTA}")
    assert share >= S.UNIQUE_SHARE


# ---------------------------------------------------------------------------------------------------------------- the exact families
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("p_exact")])
def test_exact_nucleus_rows_do_not_depend_on_top_p(name):
    for i, r in enumerate(CASES[name]):
        kept = S.topk_kept(r["x"], r["k"])
        for top_p in (r["p"] - 1e-3, r["p"], r["p"] + 1e-3):
            n_lo, n_hi = S.nucleus_band(r["x"].astype(np.float64), kept, top_p, S.DELTA)
            assert n_lo == n_hi == len(r["expect"]), f"{name} row {i} at top_p {top_p}"
            assert np.array_equal(np.sort(S.descending(r["x"], kept)[:n_lo]), r["expect"])
        want = np.zeros(len(r["x"]), bool)
        want[r["expect"]] = True
        assert S.check_nucleus(want, r["x"], kept, r["p"], S.DELTA)[3] == 0.0


def test_exact_topk_rows_have_mass_on_every_finite_kept_id():
    """`probs > 0` is the kept set only where fp32 exp does not underflow: every finite kept entry lies within 60 units of its maximum"""
    for name, rows in CASES.items():
        for r in rows:
            if r["kind"] == "exact_k":
                x = S.scaled(r["x"], r["T"])
                keep = S.expected_exact(r)
                assert keep.any() and float(x[keep].max() - x[keep].min()) < 60.0, name
