"""The premises of tests/sampler_draw_util.py, on the CPU: the host Philox reproduces the published Random123 known answers for
philox4x32-10, the u mapping and the counter / key words react to every bit they are said to carry, cdf_order is a permutation that
ascends by 256 inside a thread, admissible() behaves as documented, the exact family's rows exercise what their names say, and the
INPUT CONDITION of the GPU tolerance test holds: over the counters that test uses, at least 85 % of every case's draws admit exactly
one id at delta = 2e-5 (a condition on the inputs, computed from the float64 reference alone; a case that misses it gets other
inputs, the cap stays)."""
import numpy as np
import pytest

import sampler_draw_util as D


# ---- Philox ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key, ctr, want", [
    ((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 2, (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(key, ctr, want):
    assert D.philox4x32_10(key, ctr) == want
    assert D.philox4x32_10(key, ctr, rounds=9) != want


# ---- u ----------------------------------------------------------------------------------------------------------------------------
def test_u_is_on_the_24_bit_grid_in_the_unit_interval():
    us = [D.draw_u(seed, stream, step) for seed in (0, 7, 2 ** 40 + 1) for stream in range(40) for step in (0, 5)]
    assert all(0.0 <= u < 1.0 and (u * 2 ** 24) == int(u * 2 ** 24) for u in us)
    assert len(set(us)) == len(us)
    assert min(us) < 0.05 and max(us) > 0.95
    # word 0, shifted right by 8: not word 1, not a shift by 9
    w = D.philox4x32_10(D.key_words(7), D.counter_words(3, 5))
    assert D.draw_u(7, 3, 5) == (w[0] >> 8) / 16777216.0 and w[0] >> 8 != w[1] >> 8


def test_every_counter_and_key_word_changes_the_draw():
    seed, stream, step = 0x1234, 9, 3
    base = D.draw_u(seed, stream, step)
    assert D.counter_words(stream, step) == (9, 3, 0, 0x6d676561) and D.key_words(seed) == (0x1234, 0)
    assert D.draw_u(seed + 2 ** 32, stream, step) != base, "the seed's high half is the key's second word"
    assert D.draw_u(seed, 2 ** 32 - 1, step) != base and D.counter_words(2 ** 32 - 1, step)[0] == 0xFFFFFFFF
    assert D.draw_u(seed, stream, step + 2 ** 32) != base, "the step's high half is the counter's third word"
    assert D.counter_words(stream, 2 ** 32 + 3) == (9, 3, 1, 0x6d676561)
    assert D.draw_u(seed, step, stream) != base, "stream and step are different words"
    a, b = 0x0000000500000007, 0x0000000700000005
    assert D.key_words(a) == (7, 5) and D.key_words(b) == (5, 7) and D.draw_u(a, stream, step) != D.draw_u(b, stream, step)


def test_boundary_counters_land_on_thread_boundaries():
    rows, step = D.boundary_counters()
    us = [D.draw_u(seed, stream, step) * 256 for seed, stream in rows]
    assert all(u == int(u) for u in us) and len(rows) >= 4
    assert sum(1 for u in us if u % 64 == 0 and u > 0) >= 2, "case (a) needs u * 4 on an integer"


def test_the_test_counters_cover_what_they_claim():
    for case in range(len(D.STEPS)):
        rows, step = D.counters(case, D.B_DRAWS)
        assert len(set(rows)) == D.B_DRAWS
        assert any(seed >= 2 ** 32 for seed, _ in rows) and any(seed < 2 ** 32 for seed, _ in rows)
        assert any(stream == 2 ** 32 - 1 for _, stream in rows) and any(stream >= 2 ** 31 for _, stream in rows)
    assert any(s >= 2 ** 32 for s in D.STEPS) and 0 in D.STEPS


# ---- the CDF order ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [40, 255, 256, 257, 8324, 14336])
def test_cdf_order_is_a_thread_major_permutation(V):
    order = D.cdf_order(V)
    assert sorted(order.tolist()) == list(range(V))
    thread = order % 256
    assert bool((np.diff(thread) >= 0).all()), "threads in ascending order"
    same = np.diff(thread) == 0
    assert bool((np.diff(order)[same] == 256).all()), "inside one thread the ids ascend by 256"
    assert order[0] == 0 and (V <= 256 or order[1] == 256)


# ---- admissible -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [40, 300, 8324])
def test_admissible(V):
    rng = np.random.default_rng(V)
    p = rng.random(V) ** 8
    p[rng.random(V) < 0.3] = 0.0
    p[V - 1] = 0.0
    ids, c_before, c_incl = D.intervals(p)
    assert bool((p[ids] > 0).all()) and len(ids) == int((p > 0).sum()) and c_before[0] == 0.0 and c_incl[-1] == 1.0
    us = np.concatenate([rng.random(200), [0.0, 1 - 2.0 ** -24], c_incl[:5], c_before[1:4]])
    for u in us:
        one = D.admissible(p, u, 0.0)
        assert len(one) == 1
        at = int(np.nonzero(ids == one[0])[0][0])
        assert c_before[at] <= u < c_incl[at] or (at == len(ids) - 1 and u >= c_incl[at])
        for delta in (2e-5, 1e-3):
            got = D.admissible(p, u, delta)
            assert len(got) >= 1 and one[0] in got and bool((p[got] > 0).all())
            first = int(np.nonzero(ids == got[0])[0][0])
            assert ids[first:first + len(got)].tolist() == got.tolist(), "contiguous in cdf_order among the kept ids"
            meets = (c_before <= u + delta) & (c_incl >= u - delta)
            assert ids[meets].tolist() == got.tolist()
            # distance() says the same thing id by id
            d = D.distance(p, np.full(len(ids), u), ids)
            assert ids[d <= delta].tolist() == got.tolist()
    assert D.distance(p, [0.5, 0.5, 0.5], [V - 1, -1, V]).tolist() == [np.inf] * 3, "an id without mass, or outside the vocabulary"
    assert (D.n_admissible(p, us, 2e-5) == [len(D.admissible(p, u, 2e-5)) for u in us]).all()


# ---- the exact family -----------------------------------------------------------------------------------------------------------------
def test_exact_cases_exercise_what_they_are_named_for():
    seen = {}
    for name in D.EXACT_CASES:
        x, kept, k = D.exact_case(name)
        V = len(x)
        n = len(kept)
        assert n & (n - 1) == 0 and n >= 1
        thread, reg = kept % 256, kept // 256
        seen[name] = (V, set((thread // 64).tolist()), set(thread.tolist()), set(reg.tolist()))
        if k == 0:
            assert bool((x[kept] == 0).all()) and int(np.isfinite(x).sum()) == n
        us = np.arange(0, 2 ** 24, 2 ** 24 // 64) / 2 ** 24
        p = np.zeros(V)
        p[kept] = 1.0
        want = D.exact_expected(kept, us)
        assert want.tolist() == [int(D.admissible(p, u, 0.0)[0]) for u in us], name
    assert seen["a_one_per_wave"][1] == {0, 1, 2, 3} and len(seen["a_one_per_wave"][2]) == 4
    assert seen["b_one_wave_register0"][1:] == ({1}, set(range(64, 128)), {0})
    V, waves, threads, regs = seen["c_one_thread_36"]
    assert len(threads) == 1 and {0, (V - 1 - min(threads)) // 256} <= regs and V <= 256 * 36
    V, waves, threads, regs = seen["c_one_thread_56"]
    assert len(threads) == 1 and {0, 55} <= regs and V > 256 * 36
    assert seen["d_flat_8192"][2:] == (set(range(256)), set(range(32)))
    V, waves, threads, regs = seen["e_wide_8192_of_14336"]
    assert waves == {0, 1, 2, 3} and {0, 55} <= regs and len(threads) == 256
    assert D.exact_case("f_last_id")[1].tolist() == [8323]
    assert seen["g_v40"][1] == {0}
    assert D.exact_case("h_all_equal_top_k_64")[1].tolist() == list(range(64))


# ---- the input condition of the GPU tolerance test ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.TOLERANCE_CASES, ids=D.case_id)
def test_tolerance_inputs_mostly_admit_one_id(case):
    x, p, _ = D.tolerance_case(case)
    rows, step = D.counters(D.TOLERANCE_CASES.index(case), D.B_DRAWS)
    us = [D.draw_u(seed, stream, step) for seed, stream in rows]
    n = D.n_admissible(p, us, D.DELTA)
    share = float((n == 1).mean())
    print(f"[draw] {D.case_id(case)}: kept {int((p > 0).sum())}, share of draws with one admissible id {share:.3f}")
    assert abs(float(p.sum()) - 1.0) < 1e-12 and int(n.min()) >= 1
    assert share >= D.UNIQUE_SHARE, "other inputs for this case; the cap stays"


@pytest.mark.parametrize("V", sorted(D.ENTRY_TOLERANCE))
def test_entry_point_inputs_mostly_admit_one_id(V):
    """the same condition for the row and the counters every entry point is run on"""
    x, p, _ = D.tolerance_case(D.ENTRY_TOLERANCE[V])
    rows, step = D.entry_counters(D.B_DRAWS)
    n = D.n_admissible(p, [D.draw_u(seed, stream, step) for seed, stream in rows], D.DELTA)
    assert step >= 2 ** 32 and rows[0][0] >= 2 ** 32 and [s for _, s in rows] == list(range(D.B_DRAWS))
    assert float((n == 1).mean()) >= D.UNIQUE_SHARE and int((p > 0).sum()) >= 50
    assert len(D.exact_case(D.ENTRY_EXACT[V])[0]) == V
