"""Emotion transitions, the host side (no GPU): the host model of the rule (mgea.decoder.RowSchedule) and every refusal, the prompt
variants and thresholds of the drop-in layer on the synthetic vocabulary, and the PREMISE of tests/test_gpu_transitions.py's oracle
test on that test's own weights and prompts -- so that an engine that never switches cannot pass there."""
import numpy as np
import pytest

import transitions_util as tu
from mgea import synth

# what tests/test_gpu_transitions.py asserts against the spliced oracle (tests/test_gpu_kv_window.py: ORACLE_TOL = 2 x LOGIT_TOL;
# tests/test_gpu_f16.py: F16_LOGIT_TOL = 4e-3)
F32_BOUND = 2 * 1e-3
F16_BOUND = 2 * 4e-3


def test_bounds_are_the_gpu_tests():
    from parity_util import LOGIT_TOL
    assert F32_BOUND == 2 * LOGIT_TOL


def test_segment_at_against_a_brute_force_count():
    from mgea.decoder import RowSchedule
    rng = np.random.default_rng(5)
    assert RowSchedule().n_segments == 1 and RowSchedule().segment_at(10 ** 9) == 0
    for _ in range(200):
        n = int(rng.integers(1, 9))
        th = sorted(int(v) for v in rng.integers(0, 40, n - 1))
        sc = RowSchedule(tuple(th), int(rng.integers(0, 2)))
        sc.check(3)
        rec = sc.record()
        assert rec.n_segments == n and rec.key == sc.key and rec.reserved == 0 and list(rec.threshold)[:n - 1] == th
        assert all(v == 0 for v in list(rec.threshold)[n - 1:])
        prev = 0
        for k in range(-1, 45):
            want = sum(1 for t in th if t <= k)
            assert sc.segment_at(k) == want and 0 <= want < n and want >= prev   # a count, inside the row's variants, never falling
            prev = want
    assert [RowSchedule((3, 3, 7)).segment_at(k) for k in (2, 3, 6, 7)] == [0, 2, 2, 3]   # equal thresholds skip a segment


def test_every_refusal_names_the_row():
    from mgea.decoder import RowSampling, RowSchedule, pack_scheduled
    for sc, what in ((RowSchedule(tuple(range(8))), "n_segments 9"), (RowSchedule((5, 4)), "not ascending"),
                     (RowSchedule((-1,)), r"threshold\[0\]"), (RowSchedule((1,), 2), "key 2"), (RowSchedule((2 ** 31,)), "threshold")):
        with pytest.raises(ValueError, match=f"row 4: .*{what}"):
            sc.check(4)
    rows = [RowSampling(), RowSampling()]
    two = [[1, 2, 3], [4, 5, 6]]
    ok = pack_scheduled([two, [7, 8]], [RowSchedule((4,)), None], rows, 4)
    assert ok[0] == [[[1, 2, 3], [7, 8]], [[4, 5, 6], [7, 8]]] and ok[2] == 2 and ok[1][1] == RowSchedule()
    for segs, scheds, mb, what in (([two, [7, 8]], [RowSchedule((4, 9)), None], 4, "row 0: 2 prompt variants for a schedule of 3"),
                                   ([[[1, 2, 3], [4, 5]], [7]], [RowSchedule((4,)), None], 4, "row 0: prompt variants of different lengths"),
                                   ([[7], [list(range(65)), list(range(65))]], [None, RowSchedule((1,))], 4, "row 1: .* exceeds one page"),
                                   ([two, [7]], [RowSchedule((4,), 1), None], 4, "row 0: key 1 .* without a grammar_state"),
                                   ([two, [[]]], [RowSchedule((4,)), None], 4, "row 1: empty prompt"),
                                   ([two, [7]], [RowSchedule((4,)), None], 1, "exceed max_batch 1"),
                                   ([two, [7]], [RowSchedule((4,))], 4, "2 prompts but 1 schedules")):
        with pytest.raises(ValueError, match=what):
            pack_scheduled(segs, scheds, rows, mb)
    # a page-wide prompt is fine, and an unscheduled one may be wider
    pack_scheduled([[list(range(64)), list(range(64))], list(range(70))], [RowSchedule((1,)), None], rows, 4)


def test_transition_prompts_and_thresholds_on_the_synthetic_vocabulary():
    from generate_music.grammar import OPEN, start_state, track_grammar
    from generate_music.transitions import start_thresholds, step_thresholds, transition_prompts
    from mgea.decoder import RowSchedule
    vocab = synth.decoder_vocab(300, with_eos=True)
    prompt = ["[START_SEQUENCE]", "[BPM] 120", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]
    sets = [("[BPM] 120", "[KEY_SIGNATURE] C major"), ("[BPM] 60", "[KEY_SIGNATURE] A minor"), ("[BPM] 180", "[KEY_SIGNATURE] F# major")]
    vs = transition_prompts(prompt, sets)
    assert vs[0] == prompt and len(vs) == 3 and all(len(v) == len(prompt) and all(t in vocab for t in v) for v in vs)
    for v, (bpm, key) in zip(vs, sets):
        assert v[1] == bpm and v[2] == key and v[0] == prompt[0] and v[3:] == prompt[3:]   # the instruments stay
    for bad, what in ((prompt[:1] + prompt[2:], "exactly one"), (prompt + ["[BPM] 60"], "exactly one")):
        with pytest.raises(ValueError, match=what):
            transition_prompts(bad, sets)
    with pytest.raises(ValueError, match="outside"):
        transition_prompts(prompt, sets * 3)
    with pytest.raises(ValueError, match="pair"):
        transition_prompts(prompt, [("[KEY_SIGNATURE] C major", "[BPM] 60")])
    g = track_grammar(vocab)
    K = g.n_state - 2
    assert K == 5 and start_state(g, [vocab[t] for t in prompt]) == OPEN
    assert start_thresholds(g, [1]) == [] and step_thresholds(24, [3]) == []
    for shares in ([1, 1], [1, 1, 1], [5, 1], [1, 9], [1] * 5, [1] * 8, [100, 1, 1]):
        th = start_thresholds(g, shares)
        sc = RowSchedule(tuple(th), 1)
        sc.check()
        assert len(th) == len(shares) - 1 and all(2 + 1 <= t <= 2 + K - 1 for t in th) and th == sorted(th)
        assert sc.segment_at(0) == 0 and sc.segment_at(OPEN) == 0 and sc.segment_at(2) == 0   # HEAD, OPEN and the first class: segment 0
        assert sc.segment_at(2 + K - 1) == len(shares) - 1                                    # the last class: the last segment
        if len(shares) <= K:
            assert len(set(th)) == len(th), f"{shares}: an empty segment although the grammar has {K} classes"
    assert start_thresholds(g, [1, 1, 1]) == [4, 5] and start_thresholds(g, [1, 9]) == [3] and start_thresholds(g, [9, 1]) == [6]
    assert step_thresholds(24, [1, 2, 1]) == [6, 18] and step_thresholds(10, [1, 1, 1]) == [3, 7]
    for bad in ([], [1, 0], [1, float("inf")], [-1, 2]):
        with pytest.raises(ValueError, match="shares"):
            step_thresholds(24, bad)


def test_the_oracle_tests_premise_holds_on_its_own_inputs():
    """For the weights, prompts and forced ids tests/test_gpu_transitions.py uses, the oracle's teacher-forced log-probabilities with
    and without the spliced cache are equal before a row's first switch and differ at EVERY step from it on, by at least 10 x the
    fp32 bound and 2 x the fp16 bound that test asserts: an engine that never switches, or switches late, fails there."""
    need = max(10 * F32_BOUND, 2 * F16_BOUND)
    for f16 in (False, True):
        n_sched = 0
        for b, ((variants, th), (forced, want, plain, segs)) in enumerate(zip(tu.ROWS, tu.reference(f16))):
            assert len(forced) == tu.N_STEPS and len(variants) == len(th) + 1
            d = (want - plain).abs()
            if not th:
                assert segs == [0] * tu.N_STEPS and float(d.max()) == 0.0
                continue
            n_sched += 1
            on = th[0]
            assert segs[on] == 1 and segs[-1] == len(th) and (on == 0 or (segs[on - 1] == 0 and float(d[:on].max()) == 0.0))
            print(f"[transitions] f16={f16} row {b}: switch at step {on}, |spliced - unspliced| {float(d[on:].min()):.4f} .. {float(d[on:].max()):.4f}")
            assert float(d[on:].min()) >= need, f"f16={f16} row {b}: the splice moves step {on + int(d[on:].argmin())} by only {float(d[on:].min()):.4f}"
        assert n_sched == 6 and sorted(len(v) for v, _ in tu.ROWS[:3]) == [1, 2, 3]   # rows of 1, 2 and 3 segments in the 3-row batch too
