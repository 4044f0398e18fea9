"""The KV window's host model (mgea.decoder.KVWindow, the contract of include/mgea.h at mgea_decoder_set_window), without a GPU:
the closed form against a brute-force run of the eviction rule, the bounds on what a step attends, the host rotation, and the
validation errors."""
import numpy as np
import pytest

from mgea.decoder import KV_PAGE_TOKENS, WINDOW_MAX_RING, WINDOW_MAX_STEPS, KVWindow

PAGE = KV_PAGE_TOKENS


def geometries():
    return [(P, S) for P in range(3, 9) for S in range(1, P - 1)]


@pytest.mark.parametrize("P,S", geometries())
def test_closed_form_agrees_with_the_rule(P, S):
    w = KVWindow(S, P - S, 10 ** 6)
    assert PAGE == 64 and w.pages == P and w.tokens == 64 * P
    for Lp in range(1, 64 * S):
        i0 = w.first_eviction_step(Lp)
        assert i0 == 64 * P - 1 - Lp
        n = i0 + 3 * 64 + 2        # up to the fourth eviction
        # the count at every step; the sets themselves at the steps around every eviction and a stride of the rest
        probe = {0, 1, n - 1} | {i0 + 64 * k + d for k in range(4) for d in (-1, 0, 1, 63)} | set(range(0, n, 37))
        counts, sets = w.simulate(Lp, n, probe)
        for i in range(n):
            e = w.evictions(Lp, i)
            assert e == (0 if i < i0 else 1 + (i - i0) // 64)
            cnt = w.attended_count(Lp, i)
            assert cnt == counts[i] == Lp + i + 1 - 64 * e
            if i >= i0:
                assert 64 * P - 64 <= cnt <= 64 * P - 1, (P, S, Lp, i, cnt)
            else:
                assert cnt <= 64 * P - 1
            if i in probe:
                a, b = w.attended(Lp, i)
                assert set(a) | set(b) == sets[i], (P, S, Lp, i)
                if e:
                    assert a == range(0, 64 * S) and b == range(64 * (S + e), Lp + i + 1)
        assert set(range(Lp)) <= sets[n - 1], "the prompt never leaves"


def test_attended_count_touches_both_bounds():
    w = KVWindow(1, 2, 1000)
    i0 = w.first_eviction_step(5)
    assert w.attended_count(5, i0 - 1) == 64 * 3 - 1 and w.attended_count(5, i0) == 64 * 3 - 64
    assert w.attended_count(5, i0 + 63) == 64 * 3 - 1 and w.attended_count(5, i0 + 64) == 64 * 3 - 64


def test_host_rotation():
    B, mp, S, R = 5, 6, 2, 3
    P = S + R
    pt = np.arange(B * mp, dtype=np.int32).reshape(B, mp) + 100
    ctx = np.array([64 * P - 1, 64 * P - 2, 64 * P, 64 * P - 1, 7], np.int32)
    done = np.array([0, 0, 0, 1, 0], np.int32)
    ev = np.array([3, 0, 0, 9, 0], np.int32)
    npt, nctx, nev = KVWindow.evict_rows(pt, S, R, ctx, done, ev)
    assert npt[0].tolist() == [100, 101, 103, 104, 102, 105], "sink and the entries beyond P stay, the ring rotates left"
    assert nctx[0] == 64 * P - 65 and nev[0] == 4
    assert (npt[1:] == pt[1:]).all() and (nctx[1:] == ctx[1:]).all() and (nev[1:] == ev[1:]).all()
    assert pt[0].tolist() == list(range(100, 106)), "the inputs are not written"


def test_validation():
    KVWindow(1, 2, 1).check(192)
    KVWindow(1, 15, WINDOW_MAX_STEPS).check(1024)
    with pytest.raises(ValueError, match="ring_pages 1 "):
        KVWindow(1, 1, 10).check(1024)
    with pytest.raises(ValueError, match="sink_pages 0 "):
        KVWindow(0, 4, 10).check(1024)
    with pytest.raises(ValueError, match=f"ring_pages {WINDOW_MAX_RING + 1} "):
        KVWindow(1, WINDOW_MAX_RING + 1, 10).check(1 << 20)
    with pytest.raises(ValueError, match="sink_pages 2 \\+ ring_pages 2 exceed the 3 whole pages of max_ctx 255"):
        KVWindow(2, 2, 10).check(255)
    for bad in (0, -1, WINDOW_MAX_STEPS + 1):
        with pytest.raises(ValueError, match=f"max_steps {bad} "):
            KVWindow(1, 2, bad).check(1024)
    w = KVWindow(1, 2, 100)
    w.check_call(63, 100)
    with pytest.raises(ValueError, match="prompt width 64 \\+ 1 exceeds the window's sink of 1 pages"):
        w.check_call(64, 10)
    with pytest.raises(ValueError, match="101 steps exceed the window's max_steps 100"):
        w.check_call(5, 101)
