"""Windowed penalties over token classes on the MI355X (include/mgea.h, mgea_row_class_penalty): the kernel alone against the numpy
rule of class_penalty_util.py, bit for bit; class-penalised generations against the oracle (teacher-forced log-probabilities;
free-running greedy ids against the host's maximum of the penalised oracle row, and a hard property of the ids alone); identities
with the unpenalised calls and the step graphs; guidance pairs, blend groups, a KV window, truncation and a grammar; refusals; the
endpoint.

Tolerances are test_gpu_blend.py's for ONE row of weight 1 (W = 1): teacher-forced 4 * LOGIT_TOL, greedy 2 * 2 * LOGIT_TOL.  d, what
the rule subtracts, is an exact function of the ids; subtracting it adds one fp32 rounding of a value below 2e4 * 2^-24 ~ 1e-3 only
for |d| near 1e4, and the records below keep |d| <= 8 (rounding <= 5e-7): inside those bounds as they stand.
"""
import functools
import os
import random

import numpy as np
import pytest
import torch

from class_penalty_util import counts, host_rule
from mgea import synth
from parity_util import LOGIT_TOL
from test_gpu_guidance import grammar_of, guided_case, oracle_logps, oracle_of
from test_gpu_logprobs import make
from test_gpu_step_forms import N_STEPS, case

pytestmark = pytest.mark.gpu
N_FORCED = 12
SCORED_BOUND = 4 * 1.0 * LOGIT_TOL
GREEDY_TOL = 2 * 1.0 * 2 * LOGIT_TOL
RECORDS = ((0.5, 2.0, 4), (-0.25, 1.0, 0), (1.0, 0.0, 2))   # (frequency, presence, window) of the three rows of guided_case


def map12(vocab, holes=True):
    """class_of[i] = i % 12, every 13th id in no class"""
    m = np.arange(vocab, dtype=np.int32) % 12
    if holes:
        m[::13] = -1
    return m


def penalties(recs):
    from mgea.decoder import ClassPenalty
    return [ClassPenalty(*r) for r in recs]


def d_rows(class_of, ids, rec):
    """[len(ids), V] float64: what the rule subtracts at every step of a row that took `ids` -- host_rule on a row of zeros"""
    V, n = len(class_of), len(ids)
    hist = np.asarray([ids], dtype=np.int32)
    out = np.empty((n, V))
    for s in range(n):
        out[s] = -host_rule(np.zeros((1, V), np.float32), class_of, hist, [s], [0], [rec])[0].astype(np.float64)
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------- 1. the kernel alone
STRIDE = 4100
T_VALUES = (1, 255, 256, 257, 4095, 4096)


def op_case(rng, V, class_of, n_class, t, window):
    """B = 5: row 0 off, row 1 finished, row 2 at t = 0, row 3 with its whole window in ONE class, row 4 ordinary.  Inside [lo, t) a
    row's history holds ids of the classes [0, n_class - 1) (and of class -1); everywhere else ids of class n_class - 1, which the
    window does not otherwise hold: a wrong window is a wrong count, never an index out of range.  (n_class == 1: class 0 on both
    sides, so a wrong window is a wrong count of class 0.)"""
    by_class = [np.nonzero(class_of == c)[0] for c in range(n_class)]
    outside_ids = by_class[n_class - 1]
    inner = np.nonzero((class_of >= 0) & (class_of < max(n_class - 1, 1)))[0]
    free = np.nonzero(class_of < 0)[0]
    pool = np.concatenate([inner, free]) if len(free) else inner
    hist = rng.choice(outside_ids, size=(5, STRIDE)).astype(np.int32)
    row_step = [t, t, 0, t, t]
    done = [0, 1, 0, 0, 0]
    lo = max(0, t - window) if window > 0 else 0
    one = by_class[int(rng.integers(0, max(n_class - 1, 1)))]
    hist[3, lo:t] = rng.choice(one, size=t - lo)
    hist[4, lo:t] = rng.choice(pool, size=t - lo)
    hist[0, lo:t] = rng.choice(pool, size=t - lo)
    hist[1, lo:t] = rng.choice(pool, size=t - lo)
    recs = [(0.0, 0.0, window), (0.3, 1.0, window), (0.3, 1.0, window), (0.1, -1.25, window), (-0.7, 2.5, window)]
    return hist, row_step, done, recs


# V: fewer ids than threads, one past the block, the tiny and real vocabularies, the cap; n_class: 1, 12, 128 and V, the identity map
# (n_class <= vocab by contract: V = 31 has no 128)
OP_SHAPES = [(V, n) for V in (31, 257, 300, 8324, 14336) for n in (1, 12, 128, V) if n <= V]


@pytest.mark.parametrize("V,n_class", OP_SHAPES)
def test_op_class_penalty_equals_the_host_rule(V, n_class):
    from mgea import ops
    rng = np.random.default_rng(7000 + V + n_class)
    class_of = (np.arange(V) % n_class).astype(np.int32)
    if V >= 4 * n_class:
        class_of[rng.choice(V, size=V // 9, replace=False)] = -1   # ids in no class
        for c in range(n_class):                                   # (every class keeps an id)
            class_of[c] = c
    raw = np.empty((6, V), np.float32)
    raw[:5] = (rng.standard_normal((5, V)) * 3).astype(np.float32)
    raw[5] = np.frombuffer(np.full(V, 0x7FC0DEAD, np.uint32).tobytes(), np.float32)   # the guard row behind the batch: poison
    dev = torch.from_numpy(raw).cuda()
    pairs = {(t, w) for t in T_VALUES for w in T_VALUES + (0,)} | {(w + k, w) for w in (1, 2, 64, 1000) for k in (-1, 0, 1)}
    n_checked = 0
    for t, window in sorted(pairs):
        if t < 1:
            continue
        hist, row_step, done, recs = op_case(rng, V, class_of, n_class, t, window)
        want = host_rule(raw[:5], class_of, hist, row_step, done, recs)
        got = ops.class_penalty(dev, class_of, hist, row_step, done, penalties(recs)).cpu().numpy()
        assert got[5].tobytes() == raw[5].tobytes(), f"V={V} t={t} window={window}: the guard row behind the batch was touched"
        for b in range(5):
            assert np.array_equal(got[b], want[b]), \
                f"V={V} n_class={n_class} t={t} window={window} row {b}: {int((got[b] != want[b]).sum())} logits differ from the host rule"
        for b in (0, 1, 2):
            assert got[b].tobytes() == raw[b].tobytes(), f"row {b} (off / finished / t = 0) was written"
        assert not np.array_equal(got[3], raw[3]), "row 3 is on and its window holds a class: it was not penalised"
        if counts(hist[4], t, window, class_of, n_class).sum() > 0:   # (a short window may hold ids of class -1 alone)
            assert not np.array_equal(got[4], raw[4]), "row 4 is on and its window holds a class: it was not penalised"
        lo = max(0, t - window) if window > 0 else 0
        assert counts(hist[3], t, window, class_of, n_class).max() == t - lo, "row 3's window is one class"
        n_checked += 1
    assert n_checked == len([p for p in pairs if p[0] >= 1])
    assert dev.cpu().numpy().tobytes() == raw.tobytes(), "class_penalty works on a copy"
    with pytest.raises(ValueError, match="row 1"):
        ops.class_penalty(dev, class_of, hist, row_step, done, penalties([(0, 0, 0), (float("nan"), 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]))


# ------------------------------------------------------------------------------------------------- 2. teacher-forced, the oracle
@functools.lru_cache(maxsize=None)
def forced_reference(tag):
    """the teacher-forced oracle rows of guided_case, once per golden: per row its [12, V] float64 log_softmax matrix"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"decoder_{tag}.npz"))
    ref, vocab = oracle_of(g)
    prompts, _, forced = guided_case(vocab)
    return [oracle_logps(ref, p, f) for p, f in zip(prompts, forced)]


@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])   # unfused / fused tail
def test_class_penalized_logprobs_against_the_oracle(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    vocab = int(g["cfg"][1])
    prompts, _, forced = guided_case(vocab)
    lps = forced_reference(tag)
    class_of = map12(vocab)
    steps = torch.arange(N_FORCED)
    # power, from the oracle alone and before anything runs on the GPU: a build that penalises nothing fails
    wants, power = [], 0.0
    for b in range(3):
        ids = torch.tensor(forced[b])
        want = torch.log_softmax(lps[b] - d_rows(class_of, forced[b], RECORDS[b]), dim=1)[steps, ids]
        power = max(power, float((want - lps[b][steps, ids]).abs().max()))
        wants.append(want)
    print(f"[cpen] {tag}: penalised vs plain log-probability differs by up to {power:.3f} (needs {10 * SCORED_BOUND:.3f})")
    assert power >= 10 * SCORED_BOUND, f"{tag}: the penalised and the plain log-probabilities differ by only {power:.3f}"
    eng, _, _ = make(g, max_batch=4)
    eng.set_penalty_classes(class_of)
    rows = [RowSampling(top_k=1, eos_id=-1, class_penalty=cp) for cp in penalties(RECORDS)]
    res = eng.generate_scored(prompts, rows, N_FORCED, force_ids=forced)
    assert res.ids.cpu().tolist() == forced and res.logprobs.shape == (3, N_FORCED)
    assert eng.class_penalty_info() == dict(n_class=12, rows=3, class_penalized_steps=N_FORCED)
    for b in range(3):
        d = float((res.logprobs[b].cpu().double() - wants[b]).abs().max())
        print(f"[cpen] {tag} row {b} record {RECORDS[b]}: |logprob - oracle| {d:.2e} (bound {SCORED_BOUND:.1e})")
        assert d <= SCORED_BOUND, f"{tag} row {b}: class-penalised logprobs off the oracle by {d:.2e} > {SCORED_BOUND:.1e}"
    eng.close()


# ------------------------------------------------------------------------------------------------------ 3. greedy, free-running
def recurrences(ids, class_of, window):
    """the steps whose id has a class that one of the `window` ids before it has (ids of class -1 never count)"""
    bad = []
    for s, i in enumerate(ids):
        c = class_of[i]
        if c >= 0 and any(class_of[j] == c for j in ids[max(0, s - window):s]):
            bad.append(s)
    return bad


@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_greedy_ids_are_the_hosts_penalised_maximum(golden, tag):
    from mgea.decoder import RowSampling
    g = golden("decoder_" + tag)
    ref, vocab = oracle_of(g)
    prompts, _, _ = guided_case(vocab)
    class_of = map12(vocab)
    eng, _, _ = make(g, max_batch=4)
    eng.set_penalty_classes(class_of)
    rows = [RowSampling(top_k=1, eos_id=-1, class_penalty=cp) for cp in penalties(RECORDS)]
    ids = eng.generate_rows(prompts, rows, N_FORCED).cpu().tolist()
    assert eng.class_penalty_info() == dict(n_class=12, rows=3, class_penalized_steps=N_FORCED)
    for b in range(3):
        assert len(ids[b]) == N_FORCED and min(ids[b]) >= 0
        x = oracle_logps(ref, prompts[b], ids[b]) - d_rows(class_of, ids[b], RECORDS[b])   # [12, V]
        gap = float((x.max(dim=1).values - x[torch.arange(N_FORCED), torch.tensor(ids[b])]).max())
        print(f"[cpen] {tag} row {b}: chosen id below the host's penalised maximum by at most {gap:.2e} (bound {GREEDY_TOL:.1e})")
        assert gap <= GREEDY_TOL, f"{tag} row {b}: a greedy id is {gap:.2e} below the host's maximum of the penalised oracle row"
    eng.close()


@pytest.mark.parametrize("tag", ["tiny", "tiny8h"])
def test_no_class_recurs_inside_the_window(golden, tag):
    """presence 1e4, window 4, 12 classes over every id: the id of step s is in none of the classes of the 4 ids before it (12 > 4:
    always satisfiable; 1e4 is far above any logit difference of the model).  That is the rule's window exactly, and it contains the
    issue's property -- no class recurs within 4 consecutive ids."""
    from mgea.decoder import ClassPenalty, RowSampling
    g = golden("decoder_" + tag)
    vocab = int(g["cfg"][1])
    class_of = map12(vocab, holes=False)
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)]
    plain = [g[f"greedy{i}"].tolist()[len(p):] for i, p in enumerate(prompts)]
    for i, row in enumerate(plain):   # the premise, on the CPU: unpenalised greedy ids do repeat a class within the window
        n = len(recurrences(row, class_of, 4))
        print(f"[cpen] {tag} golden row {i}: {n} recurrences in {len(row)} unpenalised ids")
        assert n >= 1, f"{tag} golden row {i}: the unpenalised ids never repeat a class within 4: the property would show nothing"
    n_steps = min(len(r) for r in plain)
    eng, _, _ = make(g, max_batch=4)
    eng.set_penalty_classes(class_of)
    rows = [RowSampling(top_k=1, eos_id=-1, class_penalty=ClassPenalty(0.0, 1e4, 4)) for _ in prompts]
    ids = eng.generate_rows(prompts, rows, n_steps).cpu().tolist()
    for b in range(3):   # every row, every step
        assert len(ids[b]) == n_steps and min(ids[b]) >= 0
        bad = recurrences(ids[b], class_of, 4)
        assert not bad, f"{tag} row {b}: steps {bad} repeat a class of the 4 ids before them: {ids[b]}"
    eng.close()


# ------------------------------------------------------------------------------------------------------ 4. identities and graphs
def raw_class_penalized(eng, prompts, rows, cpen, n_steps, guide=None, blend=None):
    """mgea_decoder_generate_rows_class_penalized itself on equal-length prompts; cpen: None or (frequency, presence, window,
    reserved) per row.  Returns (status, message, ids)"""
    from mgea import _lib
    from mgea.decoder import pack_rows
    ids = torch.tensor(prompts, dtype=torch.int32, device="cuda").contiguous()
    B, Tp = ids.shape
    out = torch.empty(B, max(n_steps, 1), dtype=torch.int32, device="cuda")
    recs = pack_rows(rows, eng.vocab, None)
    carr = None if cpen is None else (_lib.RowClassPenalty * B)(*[_lib.RowClassPenalty(frequency=c[0], presence=c[1], window=c[2],
                                                                                          reserved=c[3] if len(c) > 3 else 0) for c in cpen])
    garr = None if guide is None else (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in guide])
    barr = None if blend is None else (_lib.RowBlend * B)(*[_lib.RowBlend(leader=l, weight=w) for l, w in blend])
    with eng._on_stream():
        rc = eng.lib.mgea_decoder_generate_rows_class_penalized(eng.h, _lib.ptr(ids), None, B, Tp, n_steps, recs, None, None, garr, None, 1,
                                                                None, _lib.ptr(out), None, None, None, barr, carr, eng._sp())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), out[:, :n_steps].cpu()


EQUAL = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16]]
NO_INFO = dict(rows=0, class_penalized_steps=0)


def test_null_and_off_records_are_the_unpenalised_call(golden):
    from mgea.decoder import ClassPenalty, RowSampling
    g = golden("decoder_tiny8h")
    eng, _, _ = make(g, max_batch=4)
    rows = [RowSampling(1.0, 20, seed=3 + b) for b in range(4)]
    want = eng.generate_rows(EQUAL, rows, N_STEPS).cpu()
    st0 = eng.stats()
    assert eng.class_penalty_info() == dict(n_class=0, **NO_INFO)
    rc, msg, ids = raw_class_penalized(eng, EQUAL, rows, None, N_STEPS)                      # NULL records, no map
    assert rc == 0 and torch.equal(ids, want), msg
    rc, msg, ids = raw_class_penalized(eng, EQUAL, rows, [(0.0, 0.0, 7)] * 4, N_STEPS)       # all-off records, no map
    assert rc == 0 and torch.equal(ids, want), msg
    eng.set_penalty_classes(map12(eng.vocab))
    assert eng.class_penalty_info() == dict(n_class=12, **NO_INFO)
    assert torch.equal(eng.generate_rows(EQUAL, rows, N_STEPS).cpu(), want)                  # a map set but unused
    off = [dataclass_replace(r, ClassPenalty(0.0, 0.0, 5)) for r in rows]
    assert torch.equal(eng.generate_rows(EQUAL, off, N_STEPS).cpu(), want)                   # ... and records that are off
    rc, msg, ids = raw_class_penalized(eng, EQUAL, rows, [(0.0, -0.0, 0)] * 4, N_STEPS)
    assert rc == 0 and torch.equal(ids, want), msg
    st = eng.stats()
    assert st["graph_instantiates"] == st0["graph_instantiates"] and st["graph_nodes"] == st0["graph_nodes"], "an unpenalised call captured a graph"
    assert eng.class_penalty_info() == dict(n_class=12, **NO_INFO)
    eng.set_penalty_classes(None)
    assert eng.class_penalty_info() == dict(n_class=0, **NO_INFO)
    assert torch.equal(eng.generate_rows(EQUAL, rows, N_STEPS).cpu(), want)
    eng.close()


def dataclass_replace(row, cp):
    import dataclasses
    return dataclasses.replace(row, class_penalty=cp)


def test_class_penalized_graphs_are_reused_and_leave_the_others_alone(golden):
    from mgea.decoder import ClassPenalty, RowSampling
    g = golden("decoder_tiny8h")
    eng, _, _ = make(g, max_batch=4)
    fresh, _, _ = make(g, max_batch=4)
    rows = [RowSampling(1.0, 20, seed=3 + b) for b in range(4)]
    before = eng.generate_rows(EQUAL, rows, N_STEPS).cpu()
    plain_inst = eng.stats()["graph_instantiates"]
    eng.set_penalty_classes(map12(eng.vocab))
    on = [dataclass_replace(r, ClassPenalty(0.5, 2.0, 4)) for r in rows]
    a = eng.generate_rows(EQUAL, on, N_STEPS).cpu()
    st = eng.stats()
    assert st["graph_instantiates"] > plain_inst, "the class-penalised steps are graphs of their own"
    assert eng.class_penalty_info() == dict(n_class=12, rows=4, class_penalized_steps=N_STEPS)
    assert not torch.equal(a, before)
    # one launch more than the unpenalised step of that batch size and form
    eng.generate_rows(EQUAL, rows, 1)
    plain_nodes = eng.stats()["graph_nodes"]
    eng.generate_rows(EQUAL, on, 1)
    assert eng.stats()["graph_nodes"] == plain_nodes + 1
    inst = eng.stats()["graph_instantiates"]
    # other values, windows and rows-on replay the cached graphs
    other = [dataclass_replace(rows[0], ClassPenalty(-0.25, 0.0, 0)), rows[1], dataclass_replace(rows[2], ClassPenalty(0.0, 3.0, 2)), rows[3]]
    b = eng.generate_rows(EQUAL, other, N_STEPS).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "other records captured a new class-penalised graph"
    assert eng.class_penalty_info() == dict(n_class=12, rows=2, class_penalized_steps=N_STEPS)
    assert not torch.equal(b[0], a[0])
    after = eng.generate_rows(EQUAL, rows, N_STEPS).cpu()
    assert eng.stats()["graph_instantiates"] == inst and eng.class_penalty_info() == dict(n_class=12, **NO_INFO)
    want = fresh.generate_rows(EQUAL, rows, N_STEPS).cpu()
    assert torch.equal(before, want) and torch.equal(after, want), "an unpenalised call next to a class-penalised one drew other ids"
    # rows that are off inside a class-penalised batch keep the ids they get in the plain batch of that size and form
    assert torch.equal(b[1], want[1]) and torch.equal(b[3], want[3])
    eng.close()
    fresh.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_graph_modes_agree(golden, tune, tag):
    from mgea.decoder import ClassPenalty, RowSampling
    g, prompts, _ = case(golden, tag)
    rows = [RowSampling(1.0, 20, seed=7, class_penalty=ClassPenalty(0.5, 2.0, 4)), RowSampling(top_k=1, class_penalty=ClassPenalty(0.0, 1e4, 3))]
    seen = None
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng, _, _ = make(g, max_batch=4)
        eng.set_penalty_classes(map12(eng.vocab, holes=False))
        ids = eng.generate_rows(prompts, rows, 2 * N_STEPS).cpu()
        assert eng.class_penalty_info()["class_penalized_steps"] == 2 * N_STEPS and int(ids.min()) >= 0
        res = eng.generate_scored(prompts, rows, 2 * N_STEPS)
        assert torch.equal(res.ids.cpu(), ids), f"{tag} {mode}: scoring changed the ids"
        assert not recurrences(ids[1].tolist(), map12(eng.vocab, holes=False), 3)
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        if seen is not None:
            assert torch.equal(ids, seen), f"{tag}: ids under {mode} differ from graphs8"
        seen = ids if seen is None else seen
        eng.close()


# --------------------------------------------------------------------------------------------------------------- 5. composition
def test_pairs_and_groups_take_their_leaders_record(golden):
    from mgea.decoder import ClassPenalty, RowSampling
    g, prompts, _ = case(golden, "tiny8h")
    vocab = int(g["cfg"][1])
    class_of = map12(vocab, holes=False)
    rng = np.random.default_rng(23)
    others = [[int(v) for v in rng.integers(0, vocab, n)] for n in (4, 3, 5)]
    eng, _, _ = make(g, max_batch=8)
    eng.set_penalty_classes(class_of)
    rows = [RowSampling(1.0, 20, seed=7, class_penalty=ClassPenalty(0.0, 1e4, 4)), RowSampling(1.0, 20, seed=8, class_penalty=ClassPenalty(0.5, 1.0, 0))]
    ids = eng.generate_guided(prompts, [p[:1] for p in prompts], rows, [1.5, 3.0], 2 * N_STEPS, all_rows=True).cpu()
    assert eng.class_penalty_info() == dict(n_class=12, rows=4, class_penalized_steps=2 * N_STEPS) and eng.guidance_info()["pairs"] == 2
    assert torch.equal(ids[2], ids[0]) and torch.equal(ids[3], ids[1]), "a shadow row left its conditional row"
    assert not recurrences(ids[0].tolist(), class_of, 4)
    ids = eng.generate_blended([[prompts[0], others[0], others[1]], [prompts[1], others[2]]], [[0.6, 0.3, 0.1], [1.5, -0.5]], rows, 2 * N_STEPS,
                               all_rows=True).cpu()
    assert eng.class_penalty_info() == dict(n_class=12, rows=5, class_penalized_steps=2 * N_STEPS) and eng.blend_info()["groups"] == 2
    for m, l in {2: 0, 3: 0, 4: 1}.items():
        assert torch.equal(ids[m], ids[l]), f"member row {m} left its leader"
    assert not recurrences(ids[0].tolist(), class_of, 4)
    # through the C ABI a shadow / member row's own record is validated and then ignored: the conditional's / the leader's is used
    rows4 = [RowSampling(1.0, 20, seed=3) for _ in EQUAL]
    hard, soft, off = (0.0, 1e4, 4), (0.25, 0.5, 0), (0.0, 0.0, 0)
    rc, msg, got = raw_class_penalized(eng, EQUAL, rows4, [hard, off, off, soft], 2 * N_STEPS, guide=[(3, 1.5), (-1, 0), (-1, 0), (-1, 0)])
    assert rc == 0 and torch.equal(got[3], got[0]) and not recurrences(got[0].tolist(), class_of, 4), msg
    rc, msg, got = raw_class_penalized(eng, EQUAL, rows4, [soft, hard, off, off], 2 * N_STEPS, blend=[(1, 0.3), (1, 0.7), (-1, 0), (-1, 0)])
    assert rc == 0 and torch.equal(got[0], got[1]) and not recurrences(got[1].tolist(), class_of, 4), msg
    eng.close()


def test_windowed_run_longer_than_the_context():
    from mgea.decoder import ClassPenalty, DecoderEngine, RowSampling
    from test_gpu_kv_window import draw_prompts, model, want_evictions
    sd, n_head, vocab = model("tiny8h")
    n_steps = 300
    eng = DecoderEngine(sd, n_head=n_head, max_batch=4, max_ctx=192)
    eng.set_window(1, 2, 320)
    class_of = (np.arange(vocab) % 128).astype(np.int32)   # 128 classes > window 64: the property is always satisfiable
    eng.set_penalty_classes(class_of)
    p = draw_prompts(6, vocab, (5, 9, 7))
    rows = [RowSampling(1.0, 20, seed=11 + b, class_penalty=ClassPenalty(0.0, 1e4, 64)) for b in range(2)]
    rows.append(RowSampling(1.0, 20, seed=13, class_penalty=ClassPenalty(0.5, 0.0, 64)))
    ids = eng.generate_rows(p, rows, n_steps).cpu()
    assert ids.shape == (3, n_steps) and int(ids.min()) >= 0, "a windowed class-penalised run returns n_steps ids"
    assert eng.class_penalty_info() == dict(n_class=128, rows=3, class_penalized_steps=n_steps)
    for b in (0, 1):   # over the whole run, far past the cache's window: the counts follow the history
        bad = recurrences(ids[b].tolist(), class_of, 64)
        assert not bad, f"row {b}: steps {bad} repeat a class of the 64 ids before them"
    assert eng.window_evictions() == want_evictions(eng.window, p, n_steps)
    assert max(eng.window_evictions()) >= 1
    # the soft row, teacher-forced on its own ids in a second run: the same ids, so the rule is a function of the history alone
    again = eng.generate_rows(p, rows, n_steps).cpu()
    assert torch.equal(again, ids)
    eng.close()


def test_with_a_truncation_and_the_track_grammar():
    from generate_music.grammar import start_state, track_grammar
    from generate_music.variety import token_classes
    from mgea.decoder import ClassPenalty, DecoderEngine, RowSampling, Truncation
    from test_gpu_kv_window import model
    sd, n_head, vocab = model("tiny8h")
    tok2id = synth.decoder_vocab(vocab, with_eos=True)
    gr = track_grammar(tok2id)
    class_of = token_classes(tok2id, "pitch_class")
    assert class_of.max() == 11 and (class_of < 0).sum() == vocab - sum(t.startswith("[NOTE]") for t in tok2id)
    eng = DecoderEngine(sd, n_head=n_head, max_batch=4, max_ctx=48)
    eng.set_grammar(gr)
    eng.set_penalty_classes(class_of)
    prompt = [tok2id[t] for t in ("[START_SEQUENCE]", "[BPM] 120", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin")]
    rows = [RowSampling(1.0, 40, seed=5 + b, grammar_state=start_state(gr, prompt), truncation=Truncation(min_p=0.02),
                        class_penalty=ClassPenalty(0.0, 1e4, 4)) for b in range(2)]
    ids = eng.generate_rows([prompt, prompt], rows, 24).cpu().tolist()
    assert eng.class_penalty_info() == dict(n_class=12, rows=2, class_penalized_steps=24) and eng.truncation_info()["steps"] == 24
    for b in range(2):
        row = [i for i in ids[b] if i >= 0]
        assert len(row) == 24 and gr.accepts(prompt + row), f"row {b} left the grammar"
        assert not recurrences(row, class_of, 4), f"row {b} repeats a pitch class within 4 notes: {row}"
        assert any(class_of[i] >= 0 for i in row)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_through_the_c_abi(golden):
    from mgea import _lib
    from mgea.decoder import ClassPenalty, RowSampling
    g = golden("decoder_tiny8h")
    eng, _, _ = make(g, max_batch=4, max_ctx=192)   # (three pages: the window below needs them)
    rows = [RowSampling(1.0, 20, seed=3) for _ in EQUAL]
    ok, off = (0.5, 1.0, 4), (0.0, 0.0, 0)
    rc, msg, _ = raw_class_penalized(eng, EQUAL, rows, [off, off, ok, off], 4)   # a row on, no map
    assert rc == _lib.EINVAL and "row 2" in msg and "no class map" in msg, msg
    eng.set_penalty_classes(map12(eng.vocab))
    rc, msg, _ = raw_class_penalized(eng, EQUAL, rows, [ok] * 4, 4)
    assert rc == 0, msg
    inst = eng.stats()["graph_instantiates"]
    for bad, who in (((float("nan"), 0.0, 4), "frequency"), ((float("inf"), 0.0, 4), "frequency"), ((1.5e4, 0.0, 4), "frequency"),
                     ((0.0, float("-inf"), 4), "presence"), ((0.0, -1.0001e4, 4), "presence"), ((0.5, 0.0, -1), "window"),
                     ((0.5, 0.0, 4097), "window"), ((0.5, 0.0, 4, 1), "reserved"), ((0.0, 0.0, 4097), "window")):
        for b in (0, 3):
            cpen = [ok] * 4
            cpen[b] = bad
            rc, msg, _ = raw_class_penalized(eng, EQUAL, rows, cpen, 4)
            assert rc == _lib.EINVAL and f"row {b}" in msg and who in msg and "decoder_generate_rows_class_penalized" in msg, (bad, rc, msg)
    assert eng.stats()["graph_instantiates"] == inst
    assert eng.class_penalty_info() == dict(n_class=12, rows=4, class_penalized_steps=4)   # a refused call enqueues and reports nothing
    # window 0 above 4096 steps needs a window (the KV window lifts the context, not this)
    eng.set_window(1, 2, 5000)
    rc, msg, _ = raw_class_penalized(eng, EQUAL, rows, [off, (0.5, 0.0, 0), off, off], 4097)
    assert rc == _lib.EINVAL and "row 1" in msg and "needs a window" in msg, msg
    eng.set_window(0)
    # the map itself
    V = eng.vocab
    for m, n_class, who in ((np.full(V, 12, np.int32), 12, "class_of[0]"), (np.full(V, -2, np.int32), 12, "class_of[0]"),
                            (np.zeros(V, np.int32), 0, "n_class"), (np.zeros(V, np.int32), V + 1, "n_class")):
        with eng._on_stream():
            rc = eng.lib.mgea_decoder_set_penalty_classes(eng.h, m.ctypes.data, n_class, eng._sp())
        assert rc == _lib.EINVAL and who in _lib.last_error(), _lib.last_error()
    assert eng.class_penalty_info()["n_class"] == 12, "a refused map left the old one"
    # the Python surface refuses the same things, naming the row
    for cp, who in ((ClassPenalty(float("nan"), 0, 4), "frequency"), (ClassPenalty(0, 2e4, 4), "presence"), (ClassPenalty(0.5, 0, 4097), "window")):
        with pytest.raises(ValueError, match=f"row 1: {who}"):
            eng.generate_rows(EQUAL, [rows[0], dataclass_replace(rows[1], cp), rows[2], rows[3]], 4)
    eng.set_penalty_classes(None)
    with pytest.raises(ValueError, match="row 1 has a class penalty but no class map"):
        eng.generate_rows(EQUAL, [rows[0], dataclass_replace(rows[1], ClassPenalty(0.5, 0, 4)), rows[2], rows[3]], 4)
    with pytest.raises(ValueError, match="class_of"):
        eng.set_penalty_classes(np.zeros(V - 1, np.int32))
    eng.close()


def test_varied_endpoint(golden, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_varied_app
    from emotion_analysis import inference
    from generate_music.variety import token_classes

    g = golden("decoder_tiny8h")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    monkeypatch.setattr(inference, "predict", lambda text: "joy")
    monkeypatch.setattr(gen, "_draw_seed", lambda: 1234)   # fixed seeds: the endpoint draws one per request

    with pytest.raises(ValueError, match="classes"):
        create_varied_app(model, seq_len=32, classes="timbre")
    with pytest.raises(ValueError, match="presence"):
        create_varied_app(model, seq_len=32, presence_penalty=float("inf"))
    with pytest.raises(ValueError, match="window"):
        create_varied_app(model, seq_len=32, presence_penalty=1.0, penalty_window=5000)
    app = create_varied_app(model, seq_len=40, temperature=1.0, top_k=20, classes="pitch_class", presence_penalty=1e4, penalty_window=4)
    served = []
    app.state.on_tokens = served.append
    text = "i am walking down a road and i see a rainbow. i love life."
    kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
    random.seed(11)
    r = TestClient(app).post("/generate", **kw)
    assert r.status_code == 200 and r.content[:4] == b"MThd"
    assert r.headers["x-emotion"] == "joy" and r.headers["x-penalty-classes"] == "pitch_class"
    assert r.headers["x-presence-penalty"] == "10000" and r.headers["x-frequency-penalty"] == "0" and r.headers["x-penalty-window"] == "4"
    n_prompt = int(r.headers["x-prompt-tokens"])
    info = model._need().class_penalty_info()
    assert info["n_class"] == 12 and info["rows"] == 1 and 0 < info["class_penalized_steps"] <= 40 - n_prompt
    assert len(served) == 1 and len(served[0]) == int(r.headers["x-generated-tokens"])
    class_of = token_classes(gen.tok2id, "pitch_class")
    new = [gen.tok2id[t] for t in served[0][n_prompt:]]
    assert len(new) >= 8 and not recurrences(new, class_of, 4), "the served piece repeats a pitch class within 4 tokens"
    # both values 0: the request runs as it always did
    app = create_varied_app(model, seq_len=40, temperature=1.0, top_k=20)
    r = TestClient(app).post("/generate", **kw)
    assert r.status_code == 200 and model._need().class_penalty_info()["rows"] == 0
