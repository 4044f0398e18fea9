"""Emotion blends -- weighted groups of rows mixed in the sampler -- on the MI355X (include/mgea.h, mgea_decoder_generate_rows_blended):
the mix kernel alone against float64 and, where the arithmetic is the same, against the guidance mix to the bit; blended generations
against the oracle run on every prompt of a group (teacher-forced log-probabilities; free-running greedy ids against the host's
blended maximum); the members and the step graphs; agreement with a guided run; refusals; a windowed blended run; the endpoint.

Tolerances are those of test_gpu_guidance.py's header per unit of W = sum_k |w_k|, the weights of the rows in g = sum_k w_k logp_k:
  op level       OP_TOL * W;
  teacher-forced 4 * W * LOGIT_TOL (each row's log-softmax: one LOGIT_TOL for the logit and one for the log-sum, weighted by |w_k|;
                 the final normalisation of g doubles that);
  greedy         2 * W * 2 * LOGIT_TOL (g at two ids, each off by at most 2 LOGIT_TOL per unit weight).
"""
import functools
import math
import os
import random

import numpy as np
import pytest
import torch

from mgea import synth
from parity_util import LOGIT_TOL
from test_gpu_guidance import grammar_of, guided_case, oracle_logps, oracle_of, row_kinds
from test_gpu_logprobs import OP_TOL, make
from test_gpu_step_forms import N_STEPS, case

pytestmark = pytest.mark.gpu
N_FORCED = 12
WEIGHTS = ((0.6, 0.3, 0.1), (1.5, -0.25, -0.25))
# the smallest |blended - leader's plain| log-probability difference over the rows of blend_case, per weight set and over both goldens,
# measured on the CPU oracle alone (test_blended_logprobs_against_the_oracle recomputes it): at least 10 x the bound of its set
POWER_FLOOR = {WEIGHTS[0]: 0.099, WEIGHTS[1]: 0.218}


def W(w):
    return float(sum(abs(v) for v in w))


def blend_case(vocab):
    """three groups of three prompts: prompt 0 of group b and the 12 forced ids are guided_case's, the other two prompts are
    default_rng(11) ids of their own (4 and 5 of them)"""
    prompts, _, forced = guided_case(vocab)
    rng = np.random.default_rng(11)
    groups = [[p] + [[int(v) for v in rng.integers(0, vocab, n)] for n in (4, 5)] for p in prompts]
    return groups, forced


@functools.lru_cache(maxsize=None)
def forced_reference(tag):
    """the teacher-forced oracle rows of blend_case, once per golden: per group its three [12, V] float64 log_softmax matrices"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"decoder_{tag}.npz"))
    ref, vocab = oracle_of(g)
    groups, forced = blend_case(vocab)
    return [[oracle_logps(ref, p, f) for p in grp] for grp, f in zip(groups, forced)]


# ------------------------------------------------------------------------------------------------------------ 1. the op alone
OP_GROUPS = {0: [0, 5], 3: [2, 3, 9], 13: [1, 4, 6, 7, 8, 10, 11, 13]}   # leader -> members, ascending; row 12 is in no group
OP_WEIGHTS = {"positive": {0: [0.7, 0.3], 3: [0.5, 0.3, 0.2], 13: [0.125] * 8},
              "negative": {0: [1.5, -0.5], 3: [1.5, -0.25, -0.25], 13: [2.0, -0.5, 0.25, -0.25, -0.5, 0.5, -0.25, -0.25]},
              "zero": {0: [1.0, 0.0], 3: [0.0, 0.6, 0.4], 13: [0.3, 0.0, 0.2, 0.0, 0.1, 0.4, 0.0, 0.0]}}


@pytest.mark.parametrize("V", [100, 8324, 9217, 14336])   # fewer ids than threads, the real vocabulary, first width past the narrow kernel, the cap
def test_op_blend_mix(V):
    from mgea import ops
    rng = np.random.default_rng(4000 + V)
    B = 14
    raw = (rng.standard_normal((B + 1, V)) * 3).astype(np.float32)   # row 14: a guard row behind the buffer the kernel is told about
    x = raw.astype(np.float64)
    logp = x - x.max(axis=1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(axis=1, keepdims=True))     # the reference, once
    dev = torch.from_numpy(raw).cuda()
    leader = [-1] * B
    for l, members in OP_GROUPS.items():
        for m in members:
            leader[m] = l
    assert leader[12] == -1 and leader[3] == 3 and leader[2] == 3 and leader[13] == 13
    worst = 0.0
    for name, sets in OP_WEIGHTS.items():
        weight = [math.nan] * B                                       # the weight of a row in no group is not read
        for l, members in OP_GROUPS.items():
            assert abs(sum(sets[l]) - 1) < 1e-12
            for m, w in zip(members, sets[l]):
                weight[m] = w
        got_t = ops.blend_mix(dev, leader, weight)
        again = ops.blend_mix(dev, leader, weight)
        assert torch.equal(got_t, again), f"V={V} {name}: two runs differ"
        got = got_t.cpu().numpy()
        assert torch.equal(dev.cpu(), torch.from_numpy(raw)), "blend_mix works on a copy"
        for l, members in OP_GROUPS.items():
            want = sum(w * logp[m] for m, w in zip(members, sets[l]))
            d = float(np.abs(got[l] - want).max())
            worst = max(worst, d / W(sets[l]))
            print(f"[blend] V={V} {name} group of {len(members)}: |g - float64| {d:.2e} (bound {OP_TOL * W(sets[l]):.1e})")
            assert d <= OP_TOL * W(sets[l]), f"V={V} {name} leader {l}: the mixed row is off float64 by {d:.2e}"
            for m in members:
                assert got[m].tobytes() == got[l].tobytes(), f"V={V} {name}: member row {m} differs from its leader's row {l}"
        assert got[12].tobytes() == raw[12].tobytes(), "a row in no group was touched"
        assert got[14].tobytes() == raw[14].tobytes(), "the guard row behind the batch was touched"
        if name == "zero":   # weights (1, 0): log_softmax(x_0) with no rounding in the combination, the pair kernel's at scale 1 to the bit
            pair = ops.guidance_mix(dev, [5] + [-1] * (B - 1), [1.0] * B).cpu().numpy()
            assert got[0].tobytes() == pair[0].tobytes(), f"V={V}: the row statistics are not reduced as guidance_mix_kernel reduces them"
    print(f"[blend] V={V}: worst |g - float64| per unit weight {worst:.2e}")
    with pytest.raises(ValueError, match="row 0"):
        ops.blend_mix(dev, [1, -1, 1], [0.5, 0, 0.5])
    with pytest.raises(ValueError, match="row 2"):
        ops.blend_mix(dev, [-1, -1, 2], [0, 0, 1.0])


# ------------------------------------------------------------------------------------------------- 2. teacher-forced, the oracle
@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])   # unfused / fused tail
def test_blended_logprobs_against_the_oracle(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    groups, forced = blend_case(int(g["cfg"][1]))
    lps = forced_reference(tag)
    steps = torch.arange(N_FORCED)
    # power, from the oracle alone and before anything runs on the GPU: the blended value is far from the leader's plain one at some
    # step, so a build that does not mix fails
    wants = {}
    for w in WEIGHTS:
        bound = 4 * W(w) * LOGIT_TOL
        assert POWER_FLOOR[w] >= 10 * bound
        for b in range(3):
            ids = torch.tensor(forced[b])
            want = torch.log_softmax(sum(wk * lp for wk, lp in zip(w, lps[b])), dim=1)[steps, ids]
            power = float((want - lps[b][0][steps, ids]).abs().max())
            print(f"[blend] {tag} group {b} weights {w}: blended vs leader's plain {power:.3f} (floor {POWER_FLOOR[w]}, bound {bound:.1e})")
            assert power >= POWER_FLOOR[w], f"{tag} group {b} weights {w}: blended and plain log-probabilities differ by only {power:.3f}"
            wants[w, b] = want
    eng, _, _ = make(g, max_batch=12)
    rows = [RowSampling(top_k=1, eos_id=-1) for _ in groups]
    for w in WEIGHTS:
        bound = 4 * W(w) * LOGIT_TOL
        res = eng.generate_blended(groups, [list(w)] * 3, rows, N_FORCED, force_ids=forced, scored=True)
        assert res.ids.cpu().tolist() == forced and res.logprobs.shape == (3, N_FORCED)
        assert eng.blend_info() == dict(groups=3, rows=9, blended_steps=N_FORCED)
        for b in range(3):
            d = float((res.logprobs[b].cpu().double() - wants[w, b]).abs().max())
            print(f"[blend] {tag} group {b} weights {w}: |logprob - oracle| {d:.2e} (bound {bound:.1e})")
            assert d <= bound, f"{tag} group {b} weights {w}: blended logprobs off the oracle by {d:.2e} > {bound:.1e}"
    eng.close()


# ------------------------------------------------------------------------------------------------------ 3. greedy, free-running
@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_blended_greedy_ids_are_the_hosts_blended_maximum(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    ref, _ = oracle_of(g)
    eng, _, _ = make(g, max_batch=12)
    groups, _ = blend_case(eng.vocab)
    weights = [WEIGHTS[0], WEIGHTS[1], WEIGHTS[0]]
    rows = [RowSampling(top_k=1, eos_id=-1) for _ in groups]
    ids = eng.generate_blended(groups, [list(w) for w in weights], rows, N_FORCED).cpu().tolist()
    assert eng.blend_info() == dict(groups=3, rows=9, blended_steps=N_FORCED)
    for b, w in enumerate(weights):
        assert len(ids[b]) == N_FORCED and min(ids[b]) >= 0
        gh = sum(wk * oracle_logps(ref, p, ids[b]) for wk, p in zip(w, groups[b]))   # [12, V]
        gap = float((gh.max(dim=1).values - gh[torch.arange(N_FORCED), torch.tensor(ids[b])]).max())
        tol = 2 * W(w) * 2 * LOGIT_TOL
        print(f"[blend] {tag} group {b} weights {w}: chosen id below the host's blended maximum by at most {gap:.2e} (bound {tol:.1e})")
        assert gap <= tol, f"{tag} group {b} weights {w}: a greedy id is {gap:.2e} below the host's blended maximum"
    eng.close()


# -------------------------------------------------------------------------------------------------- 4. members and graph modes
@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_members_take_their_leaders_ids_in_every_graph_mode(golden, tune, tag):
    from mgea.decoder import RowSampling, Truncation
    g, prompts, bias = case(golden, tag)
    vocab = int(g["cfg"][1])
    rng = np.random.default_rng(23)
    others = [[int(v) for v in rng.integers(0, vocab, n)] for n in (4, 3, 5)]
    groups = [[prompts[0], others[0], others[1]], [prompts[1], others[2]]]   # B = 5: rows 0 1 | 2 3 (group 0) 4 (group 1)
    weights = [[0.6, 0.3, 0.1], [1.5, -0.5]]
    lead = {2: 0, 3: 0, 4: 1}
    kinds = row_kinds(vocab, bias)
    kinds["truncated"] = RowSampling(1.0, 20, None, 1.2, seed=7, truncation=Truncation(min_p=0.05, typical_p=0.9))
    seen = {}
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng, _, _ = make(g, max_batch=8)
        eng.set_grammar(grammar_of(eng.vocab))
        for kind, row in kinds.items():
            rows = [row for _ in groups]
            ids = eng.generate_blended(groups, weights, rows, N_STEPS, all_rows=True).cpu()
            assert ids.shape == (5, N_STEPS) and eng.blend_info() == dict(groups=2, rows=5, blended_steps=N_STEPS)
            for m, l in lead.items():
                assert torch.equal(ids[m], ids[l]), f"{tag} {mode} {kind}: member row {m} left its leader"
            assert int(ids[:, 0].min()) >= 0
            res = eng.generate_blended(groups, weights, rows, N_STEPS, scored=True, all_rows=True)
            assert torch.equal(res.ids.cpu(), ids), f"{tag} {mode} {kind}: scoring changed the blended ids"
            for m, l in lead.items():
                assert torch.equal(res.logprobs[m], res.logprobs[l]) and torch.equal(res.choice_logprobs[m], res.choice_logprobs[l])
            if kind == "grammar":
                gr = grammar_of(eng.vocab)
                for b in range(2):
                    assert gr.accepts([int(v) for v in ids[b].tolist() if v >= 0]), f"{tag} {mode}: row {b} left the grammar"
                st = eng.grammar_states().cpu().tolist()
                assert [st[m] for m in lead] == [st[l] for l in lead.values()]
            if kind == "truncated":
                assert eng.truncation_info()["steps"] == N_STEPS
            if kind != "sampled":
                pres = eng.presence().cpu()
                for m, l in lead.items():
                    assert torch.equal(pres[m], pres[l]), "a group's penalty set is the leader's"
                assert bool(pres[2, prompts[0]].all())
            if kind in seen:
                assert torch.equal(ids, seen[kind]), f"{tag}: {kind} ids under {mode} differ from graphs8"
            seen.setdefault(kind, ids)
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        eng.close()


# ------------------------------------------------------------------------------------------ 5. the same arithmetic as guidance
def test_a_blend_of_weights_1_0_0_draws_the_ids_of_guidance_at_scale_1(golden):
    """g = 1 * logp(p) + 0 * ... in both: no rounding in the combination, so the two launches leave the same bits in row 0, and the
    same seed draws the same ids.  Both runs are three rows with the same three prompts in the same places (the decode attention's
    form depends on the batch size)."""
    from mgea.decoder import RowSampling
    g = golden("decoder_tiny8h")
    vocab = int(g["cfg"][1])
    rng = np.random.default_rng(31)
    p, q1, q2 = ([int(v) for v in rng.integers(0, vocab, 5)] for _ in range(3))
    row = RowSampling(0.9, None, 0.9, seed=2024)
    eng, _, _ = make(g, max_batch=4)
    blended = eng.generate_blended([[p, q1, q2]], [[1.0, 0.0, 0.0]], [row], 24, all_rows=True).cpu()
    assert eng.blend_info() == dict(groups=1, rows=3, blended_steps=24)
    guided = eng.generate_guided([p, q1], [q2, None], [row, row], 1.0, 24, all_rows=True).cpu()   # rows: p, q1 (filler), q2 (shadow)
    assert eng.guidance_info() == dict(pairs=1, guided_steps=24) and eng.blend_info() == dict(groups=0, rows=0, blended_steps=0)
    assert blended.shape == guided.shape == (3, 24) and int(blended.min()) >= 0
    assert torch.equal(blended[0], guided[0]), "weights (1, 0, 0) and guidance at scale 1 drew other ids from the same seed"
    assert torch.equal(blended[1], blended[0]) and torch.equal(blended[2], blended[0]) and torch.equal(guided[2], guided[0])
    assert len(set(blended[0].tolist())) > 1   # (a sampled run, not a constant one)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6. graphs
def raw_blended(eng, prompts, rows, blend, n_steps, guide=None, sched=None, n_seg_max=1):
    """mgea_decoder_generate_rows_blended itself on equal-length prompts (n_seg_max variants of them for a scheduled call); returns
    (status, message, ids)"""
    from mgea import _lib
    from mgea.decoder import pack_rows
    ids = torch.tensor([prompts] * n_seg_max if n_seg_max > 1 else prompts, dtype=torch.int32, device="cuda").contiguous()
    B, Tp = ids.shape[-2:]
    out = torch.empty(B, max(n_steps, 1), dtype=torch.int32, device="cuda")
    recs = pack_rows(rows, eng.vocab, n_steps)
    barr = None if blend is None else (_lib.RowBlend * B)(*[_lib.RowBlend(leader=l, weight=w) for l, w in blend])
    garr = None if guide is None else (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in guide])
    with eng._on_stream():
        rc = eng.lib.mgea_decoder_generate_rows_blended(eng.h, _lib.ptr(ids), None, B, Tp, n_steps, recs, None, None, garr, sched, n_seg_max,
                                                        None, _lib.ptr(out), None, None, None, barr, eng._sp())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), out[:, :n_steps].cpu()


def test_blended_graphs_are_reused_and_leave_the_unblended_ones_alone(golden):
    from mgea.decoder import RowSampling
    g, prompts, _ = case(golden, "tiny8h")
    vocab = int(g["cfg"][1])
    rng = np.random.default_rng(41)
    extra = [[int(v) for v in rng.integers(0, vocab, n)] for n in (3, 4, 5)]
    rows = [RowSampling(1.0, 20, seed=7 + b) for b in range(2)]
    eng, _, _ = make(g, max_batch=8)
    fresh, _, _ = make(g, max_batch=8)
    five = prompts + extra
    rows5 = rows + [rows[0], rows[0], rows[1]]
    before = eng.generate_rows(five, rows5, N_STEPS).cpu()
    unblended = eng.stats()["graph_instantiates"]
    a = eng.generate_blended([[prompts[0], extra[0], extra[1]], [prompts[1], extra[2]]], [[0.6, 0.3, 0.1], [0.5, 0.5]], rows, N_STEPS,
                             all_rows=True).cpu()   # B = 5
    st = eng.stats()
    assert st["graph_instantiates"] > unblended, "the blended steps are graphs of their own"
    assert eng.blend_info() == dict(groups=2, rows=5, blended_steps=N_STEPS) and st["graph_replays"] == N_STEPS
    # one launch more than the unblended step of that batch size and form
    eng.generate_rows(five, rows5, 1)
    plain_nodes = eng.stats()["graph_nodes"]
    eng.generate_blended([[prompts[0], extra[0], extra[1]], [prompts[1], extra[2]]], [[0.6, 0.3, 0.1], [0.5, 0.5]], rows, 1)
    assert eng.stats()["graph_nodes"] == plain_nodes + 1
    inst = eng.stats()["graph_instantiates"]
    # other groups and weights (one group of four and a plain row, B = 5 again) replay the cached graphs
    b = eng.generate_blended([[prompts[0], extra[0], extra[1], extra[2]], [prompts[1]]], [[2.0, -0.5, -0.25, -0.25], [1.0]], rows, N_STEPS,
                             all_rows=True).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "other groups / weights captured a new blended graph"
    assert eng.blend_info() == dict(groups=1, rows=4, blended_steps=N_STEPS)
    assert all(torch.equal(a[m], a[l]) for m, l in ((2, 0), (3, 0), (4, 1))) and all(torch.equal(b[m], b[0]) for m in (2, 3, 4))
    assert not torch.equal(a[:2], b[:2])
    after = eng.generate_rows(five, rows5, N_STEPS).cpu()
    assert eng.stats()["graph_instantiates"] == inst and eng.blend_info() == dict(groups=0, rows=0, blended_steps=0)
    want = fresh.generate_rows(five, rows5, N_STEPS).cpu()
    assert torch.equal(before, want) and torch.equal(after, want), "an unblended call next to a blended one drew other ids"
    # groups of one prompt each ARE the unblended call
    assert torch.equal(eng.generate_blended([[p] for p in five], [[1.0]] * 5, rows5, N_STEPS).cpu(), want)
    assert eng.stats()["graph_instantiates"] == inst
    eng.close()
    fresh.close()


def test_a_pair_and_a_group_in_one_batch(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_tiny8h")
    eng, _, _ = make(g, max_batch=6)
    equal = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16], [17, 18, 19], [5, 20, 21]]
    rows = [RowSampling(1.0, 20, seed=3 + b) for b in range(6)]
    plain = eng.generate_rows(equal, rows, N_STEPS).cpu()   # the unblended, unguided batch of that size and form
    guide = [(5, 2.0)] + [(-1, 0.0)] * 5
    blend = [(-1, 0.0), (2, 0.3), (2, 0.6), (2, 0.1), (-1, 0.0), (-1, 0.0)]   # the leader is the group's middle row
    rc, msg, got = raw_blended(eng, equal, rows, blend, N_STEPS, guide=guide)
    assert rc == 0, msg
    assert eng.blend_info() == dict(groups=1, rows=3, blended_steps=N_STEPS) and eng.guidance_info() == dict(pairs=1, guided_steps=N_STEPS)
    assert torch.equal(got[5], got[0]), "the shadow row left its conditional row"
    assert torch.equal(got[1], got[2]) and torch.equal(got[3], got[2]), "a member left its leader"
    assert torch.equal(got[4], plain[4]), "the ungrouped, unpaired row drew other ids than in the plain batch"
    assert not torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])
    # every leader -1 IS the truncated call
    rc, msg, ids = raw_blended(eng, equal, rows, [(-1, math.nan)] * 6, N_STEPS)
    assert rc == 0 and torch.equal(ids, plain) and eng.blend_info() == dict(groups=0, rows=0, blended_steps=0), msg
    rc, msg, ids = raw_blended(eng, equal, rows, None, N_STEPS)
    assert rc == 0 and torch.equal(ids, plain), msg
    eng.close()


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_through_the_c_abi(golden):
    from mgea import _lib
    from mgea.decoder import RowSampling, RowSchedule
    g, prompts, _ = case(golden, "tiny8h")
    eng, _, _ = make(g, max_batch=5)
    equal = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16]]
    rows = [RowSampling(1.0, 20, seed=3) for _ in equal]
    off = (-1, 0.0)
    for blend, who in (([(0, 0.5), (0, 0.5), (4, 1.0), off], "row 2"), ([(0, 0.5), (0, 0.5), (-2, 1.0), off], "row 2"),
                       ([off, (2, 0.5), off, (2, 0.5)], "row 1"), ([off, off, off, (3, 1.0)], "row 3"),
                       ([(0, 0.5), off, (0, math.nan), off], "row 2"), ([(0, 0.5), off, (0, math.inf), off], "row 2"),
                       ([off, (1, 0.5), (1, 0.4), off], "row 1"), ([off, (1, 0.5), (1, 0.6), off], "row 1")):
        rc, msg, _ = raw_blended(eng, equal, rows, blend, 4)
        assert rc == _lib.EINVAL and who in msg and "decoder_generate_rows_blended" in msg, (blend, rc, msg)
    five = equal + [[1, 2, 3]]
    rc, msg, _ = raw_blended(eng, five, rows + rows[:1], [(0, 0.2)] * 5, 4)   # (the same check with nine rows: tests/native/blend_plan_test.cpp)
    assert rc == 0, msg
    # a grouped row in a guidance pair, on either side
    rc, msg, _ = raw_blended(eng, equal, rows, [(0, 0.5), (0, 0.5), off, off], 4, guide=[(3, 1.5), (-1, 0), (-1, 0), (-1, 0)])
    assert rc == _lib.EINVAL and "row 0" in msg and "guidance pair" in msg
    rc, msg, _ = raw_blended(eng, equal, rows, [(0, 0.5), (0, 0.5), off, off], 4, guide=[(-1, 0), (-1, 0), (1, 1.5), (-1, 0)])
    assert rc == _lib.EINVAL and "row 1" in msg and "guidance pair" in msg
    # a scheduled grouped row
    sched = (_lib.RowSchedule * 4)(*[RowSchedule((2,) if b == 1 else ()).record() for b in range(4)])
    rc, msg, _ = raw_blended(eng, equal, rows, [(0, 0.5), (0, 0.5), off, off], 4, sched=sched, n_seg_max=2)
    assert rc == _lib.EINVAL and "row 1" in msg and "segments" in msg, msg
    # a capped blended call: 3 + max_ctx > max_ctx
    rc, msg, _ = raw_blended(eng, equal, rows, [(0, 0.5), (0, 0.5), off, off], eng.max_ctx)
    assert rc == _lib.ECAPACITY and "capped" in msg
    assert eng.blend_info() == dict(groups=1, rows=5, blended_steps=4)   # a refused call enqueues and reports nothing: the five-row run's figures
    with pytest.raises(ValueError, match="never capped"):
        eng.generate_blended([[equal[0], equal[1]]], [[0.5, 0.5]], rows[:1], eng.max_ctx)
    with pytest.raises(ValueError, match="group 1: its member row 5 does not fit"):
        eng.generate_blended([equal[:3], equal[:3]], [[0.5, 0.25, 0.25]] * 2, rows[:2], 4)
    with pytest.raises(ValueError, match="row 0: the weights of its group sum to 0.9"):
        eng.generate_blended([equal[:2]], [[0.5, 0.4]], rows[:1], 4)
    with pytest.raises(ValueError, match="force_ids need scored"):
        eng.generate_blended([equal[:2]], [[0.5, 0.5]], rows[:1], 4, force_ids=[[1]])
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 8. the window
def test_windowed_blended_run_longer_than_the_context():
    from mgea.decoder import RowSampling
    from test_gpu_kv_window import draw_prompts, make as make_windowed, model, want_evictions
    n_steps, max_ctx = 400, 192
    eng = make_windowed("tiny8h", max_ctx, max_batch=4, max_steps=n_steps)
    p = draw_prompts(6, model("tiny8h")[2], (5, 9, 7, 3))
    rows = [RowSampling(1.0, 20, seed=11), RowSampling(1.0, 20, seed=12)]
    ids = eng.generate_blended([[p[0], p[1], p[2]], [p[3]]], [[0.6, 0.3, 0.1], [1.0]], rows, n_steps, all_rows=True).cpu()
    assert ids.shape == (4, n_steps) and int(ids.min()) >= 0, "a windowed blended run returns n_steps ids"
    assert torch.equal(ids[2], ids[0]) and torch.equal(ids[3], ids[0]) and not torch.equal(ids[1], ids[0])
    assert eng.window_evictions() == want_evictions(eng.window, [p[0], p[3], p[1], p[2]], n_steps)   # every row on the schedule of its own prompt
    assert eng.blend_info() == dict(groups=1, rows=3, blended_steps=n_steps)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 9. the app
def test_blended_endpoint(golden, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_blended_app
    from emotion_analysis import inference

    g = golden("decoder_tiny8h")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    asked = []

    def top_k_labels(text, k=3):   # the classifier, stubbed: three labels, the last one just above min_prob
        asked.append((text, k))
        return [("joy", 0.55), ("sadness", 0.3), ("love", 0.06)][:k]
    monkeypatch.setattr(inference, "predict_top_k_labels", top_k_labels)
    monkeypatch.setattr(gen, "_draw_seed", lambda: 1234)   # fixed seeds: the endpoint draws one per request

    small = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=2)
    with pytest.raises(ValueError, match="max_batch=2 is too small"):
        create_blended_app(small, seq_len=32)
    app = create_blended_app(model, seq_len=32, temperature=1.0, top_k=20)
    served = []
    app.state.on_tokens = served.append
    client = TestClient(app)
    text = "i am walking down a road and i see a rainbow. i love life."
    kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
    random.seed(11)
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and r.content[:4] == b"MThd"
    assert asked == [(text, 3)]
    assert r.headers["x-emotion"] == "joy" and r.headers["x-emotions"] == "joy,sadness,love"
    ws = [float(v) for v in r.headers["x-blend-weights"].split(",")]
    assert ws == pytest.approx([0.55 / 0.91, 0.3 / 0.91, 0.06 / 0.91], abs=1e-4) and abs(sum(ws) - 1) < 1e-3
    info = model._need().blend_info()   # (the steps: all of them, or fewer in whole polls of 16 once the group has drawn [END_SEQUENCE])
    assert info["groups"] == 1 and info["rows"] == 3 and 0 < info["blended_steps"] <= 32 - int(r.headers["x-prompt-tokens"])
    assert len(served) == 1 and len(served[0]) == int(r.headers["x-generated-tokens"])
    # a label below min_prob goes; under guidance the unconditional prompt is one more member
    app = create_blended_app(model, seq_len=32, temperature=1.0, top_k=20, min_prob=0.1, guidance_scale=1.5)
    r = TestClient(app).post("/generate", **kw)
    assert r.status_code == 200 and r.headers["x-emotions"] == "joy,sadness" and r.headers["x-guidance-scale"] == "1.5"
    ws = [float(v) for v in r.headers["x-blend-weights"].split(",")]
    assert ws == pytest.approx([1.5 * 0.55 / 0.85, 1.5 * 0.3 / 0.85, -0.5], abs=1e-4)
    assert model._need().blend_info()["rows"] == 3
