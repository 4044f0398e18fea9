"""Emotion transitions on the MI355X (include/mgea.h, mgea_row_schedule): the two kernels alone against a host model of the store's
layout (bit patterns, the whole pool compared), a scheduled row against generate_scored run from the variant it switched to (bit-equal,
every graph mode), teacher-forced log-probabilities against the oracle with its cache spliced at the rule's steps (f32 and fp16,
split and plain attention, step-index and grammar-state keys), the compositions (window, guidance, penalty / bias / grammar rows),
graph reuse, refusals and the endpoint.

Tolerances: ORACLE_TOL = 2 x parity_util.LOGIT_TOL on a log-probability for an f32 engine (tests/test_gpu_kv_window.py) and
2 x test_gpu_f16.F16_LOGIT_TOL for an fp16 engine against the oracle on the rounded matrices.  tests/test_transitions_host.py asserts
on the CPU that the splice moves every compared value by at least 10 x / 2 x those bounds.
Observed on an MI355X: see DESIGN.md §5, "Emotion transitions"."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import transitions_util as tu
from mgea import synth
from test_gpu_f16 import F16_LOGIT_TOL
from test_gpu_kv_window import ORACLE_TOL

pytestmark = pytest.mark.gpu
PAGE = 64


# ------------------------------------------------------------------------------------------------------- 1. the kernels alone
def bits(shape, dtype, seed):
    """a tensor of `dtype` whose elements are random bit patterns (NaNs included: everything is compared as integers)"""
    it = torch.int32 if dtype == torch.float32 else torch.int16
    info = torch.iinfo(it)
    g = torch.Generator().manual_seed(seed)
    return torch.randint(info.min, info.max, shape, generator=g, dtype=torch.int64).to(it).view(dtype)


def as_int(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def host_slot(page_kv, H, dh, G, n):
    """positions [0, n) of a row's page pair [2, H, 64 * dh] (integers) as the store holds them (mgea_op_recondition): K groups
    (h, dg, t), then V groups (h, t, dg)"""
    D = dh // G
    k = page_kv[0].reshape(H, D, PAGE, G)[:, :, :n, :].reshape(-1)
    v = page_kv[1].reshape(H, PAGE, D, G)[:, :n, :, :].reshape(-1)
    return np.concatenate([k, v])


def host_apply(page_kv, slot, H, dh, G, n):
    D = dh // G
    half = H * D * n * G
    out = page_kv.copy()
    out[0].reshape(H, D, PAGE, G)[:, :, :n, :] = slot[:half].reshape(H, D, n, G)
    out[1].reshape(H, PAGE, D, G)[:, :n, :, :] = slot[half:2 * half].reshape(H, n, D, G)
    return out


@pytest.mark.parametrize("table", [False, True], ids=["computed", "table"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("dh", [32, 64, 96])
def test_recondition_kernels_against_the_host_layout(dh, dtype, table):
    from mgea import ops
    from mgea.decoder import RowSchedule
    L, n_pages, H, B, n_seg = 2, 5, 2, 3, 3
    G = 4 if dtype == torch.float32 else 8
    pages = [3, 0, 4] if table else [0, 1, 2]
    pt = torch.tensor([[p, 1] for p in pages], dtype=torch.int32) if table else None
    # row 0 switches (step 5 of thresholds 2, 4: segment 2), row 1 stands (segment 1 already), row 2 is finished and would switch
    scheds = [RowSchedule((2, 4)), RowSchedule((3, 9)), RowSchedule((1,))]
    for n in (1, 5, 16, 63, 64):
        lens = [n, max(n - 1, 1), n]
        slot_tokens = min(PAGE, n + 3)
        pool = bits((L, n_pages, 2, H, PAGE * dh), dtype, 100 * dh + n)
        store = bits((n_seg, L, B, 2 * H * dh * slot_tokens), dtype, 7 + n)
        p0, s0 = as_int(pool), as_int(store)
        for key in (0, 1):   # the same switch by the step index and by the grammar state
            sc = [RowSchedule(scheds[0].thresholds, key)] + scheds[1:]
            got_pool, got_store, cur, switches = ops.recondition(pool, store, lens, pt, schedules=sc, done=[0, 0, 1],
                                                                 row_step=[5, 5, 5] if key == 0 else [0, 5, 5],
                                                                 gram_state=[-1, -1, -1] if key == 0 else [5, 0, 0], cur_seg=[0, 1, 0])
            want = p0.copy()
            for l in range(L):
                want[l, pages[0]] = host_apply(p0[l, pages[0]], s0[2, l, 0], H, dh, G, lens[0])
            assert np.array_equal(as_int(got_pool), want), f"dh {dh} len {n} key {key}: the pool differs from the host model"
            assert int((want != p0).sum()) > 0 and np.array_equal(as_int(got_store), s0)
            assert cur.cpu().tolist() == [2, 1, 0] and switches == 1
            assert np.array_equal(as_int(pool), p0), "recondition works on copies"
        # gather alone: the slots of segment 1 hold the rows' positions, every other group of the store is untouched
        _, got_store, _, _ = ops.recondition(pool, store, lens, pt, gather_seg=1)
        want_s = s0.copy()
        for l in range(L):
            for b in range(B):
                sl = host_slot(p0[l, pages[b]], H, dh, G, lens[b])
                want_s[1, l, b, :sl.size] = sl
        assert np.array_equal(as_int(got_store), want_s), f"dh {dh} len {n}: the gathered store differs from the host model"
        # gather, then apply what was gathered: the identity on the pool, while the rows' segments move
        same, _, cur, switches = ops.recondition(pool, store, lens, pt, gather_seg=1, schedules=[RowSchedule((0,))] * 3)
        assert np.array_equal(as_int(same), p0), f"dh {dh} len {n}: gather + apply is not the identity"
        assert cur.cpu().tolist() == [1, 1, 1] and switches == 3


def test_recondition_op_refusals():
    from mgea import _lib, ops
    from mgea.decoder import RowSchedule
    pool = torch.zeros(1, 3, 2, 2, PAGE * 32)
    store = torch.zeros(2, 1, 2, 2 * 2 * 32 * 8)
    for kw, what in ((dict(pool=torch.zeros(1, 3, 2, 2, PAGE * 48), store=torch.zeros(2, 1, 2, 2 * 2 * 48 * 8), gather_seg=0), "head_dim 48"),
                     (dict(gather_seg=2), "gather_seg 2"), (dict(), "neither a gather nor an apply"),
                     (dict(store=torch.zeros(9, 1, 2, 2 * 2 * 32 * 8), gather_seg=0), "n_seg_max 9")):
        args = dict(pool=pool, store=store, lens=[3, 8], gather_seg=-1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=what) as ei:
            ops.recondition(**args)
        assert type(ei.value) is RuntimeError, f"MGEA_EINVAL expected, got {ei.value!r}"
    for kw, what in ((dict(lens=[3, 9]), "lens"), (dict(lens=[3]), "does not fit"), (dict(page_table=[[0], [3]]), "page_table"),
                     (dict(schedules=[RowSchedule()]), "1 schedules")):
        args = dict(pool=pool, store=store, lens=[3, 8], gather_seg=0)
        args.update(kw)
        with pytest.raises(RuntimeError, match=what):
            ops.recondition(**args)
    assert _lib.EINVAL == -1


# ------------------------------------------------------------------------------- 2. the engine against itself, to the bit
def make(tag="tiny8h", max_batch=4, max_ctx=None, **kw):
    from mgea.decoder import DecoderEngine
    sd, n_head, _ = tu.model(tag)
    seq_len = int(np.asarray(sd["pos"]).shape[0])
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, **kw)


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])   # fused / unfused tail
def test_a_row_switched_before_its_first_step_is_the_variants_own_generation(tune, tag):
    from mgea.decoder import RowSampling, RowSchedule
    first, variant, other = [1, 5, 9, 20, 21], [1, 6, 11, 20, 21], [3, 7, 20]   # the variant shares the first prompt's last token
    rows = [RowSampling(1.0, 20, seed=7), RowSampling(1.0, 20, seed=8)]
    n = 19
    for mode in ("graphs8", "graphs1", "nograph"):
        tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
        tune("decoder_graph_steps", 1 if mode == "graphs1" else 8)
        eng = make(tag)
        want = eng.generate_scored([variant, other], rows, n)
        stay = eng.generate_scored([first, other], rows, n)
        got = eng.generate_scheduled([[first, variant], other], rows, [RowSchedule((0,)), None], n, scored=True)
        assert eng.schedule_info() == dict(scheduled_steps=n, switches=1) and eng.segments().cpu().tolist() == [1, 0]
        for name in ("ids", "logprobs", "choice_logprobs"):
            g, w = getattr(got, name).cpu(), getattr(want, name).cpu()
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f"{tag} {mode}: {name} differ from the variant's own generation"
        assert not torch.equal(got.logprobs[0].cpu(), stay.logprobs[0].cpu()), "the unswitched generation gives the same values: no power"
        assert torch.equal(got.logprobs[1].cpu(), stay.logprobs[1].cpu())
        # a threshold beyond the call: scheduled steps, no switch, the first prompt's own generation
        late = eng.generate_scheduled([[first, variant], other], rows, [RowSchedule((n,)), None], n, scored=True)
        assert eng.schedule_info() == dict(scheduled_steps=n, switches=0) and eng.segments().cpu().tolist() == [0, 0]
        assert torch.equal(late.ids.cpu(), stay.ids.cpu()) and torch.equal(late.logprobs.cpu(), stay.logprobs.cpu())
        # the greedy form takes the launch too (no logits row is needed)
        greedy = [RowSampling(top_k=1), RowSampling(top_k=1)]
        assert torch.equal(eng.generate_scheduled([[first, variant], other], greedy, [RowSchedule((0,)), None], n).cpu(),
                           eng.generate_rows([variant, other], greedy, n).cpu()), f"{tag} {mode}: greedy"
        assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
        eng.close()


# ----------------------------------------------------------------------------------------------- 3. against the spliced oracle
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("n_rows", [3, 9], ids=["3rows-split", "9rows-plain"])
def test_teacher_forced_logprobs_against_the_spliced_oracle(n_rows, dtype):
    from mgea.decoder import RowSampling
    f16 = dtype == "f16"
    bound = 2 * F16_LOGIT_TOL if f16 else ORACLE_TOL
    ref = tu.reference(f16)[:n_rows]
    eng = make(max_batch=n_rows, max_ctx=384, dtype=dtype)   # 6 pages: 3 rows x 8 heads take the split attention, 9 rows the plain one
    segs = [v if len(v) > 1 else v[0] for v, _ in tu.ROWS[:n_rows]]
    forced = [r[0] for r in ref]
    res = eng.generate_scheduled(segs, [RowSampling(top_k=1) for _ in segs], tu.schedules()[:n_rows], tu.N_STEPS, scored=True,
                                 force_ids=forced)
    assert res.ids.cpu().tolist() == forced
    want_seg = [r[3][-1] for r in ref]
    assert eng.segments().cpu().tolist() == want_seg
    assert eng.schedule_info() == dict(scheduled_steps=tu.N_STEPS, switches=sum(sum(1 for a, c in zip([0] + r[3][:-1], r[3]) if a != c) for r in ref))
    worst = 0.0
    for b, (_, want, plain, _) in enumerate(ref):
        d = float((res.logprobs[b].cpu().double() - want).abs().max())
        off = float((res.logprobs[b].cpu().double() - plain).abs().max())
        worst = max(worst, d)
        print(f"[transitions] {dtype} B {n_rows} row {b}: |logprob - spliced oracle| {d:.2e} (bound {bound:.1e}; from the unspliced oracle {off:.2e})")
        assert d <= bound, f"{dtype} B {n_rows} row {b}: off the spliced oracle by {d:.2e} > {bound:.1e}"
    print(f"[transitions] {dtype} B {n_rows}: worst |logprob - spliced oracle| {worst:.2e}")
    eng.close()


def grammar_case():
    """The track grammar of the synthetic vocabulary, a prompt that ends in OPEN, and forced ids that walk the START classes up, open
    a second track and walk up again; thresholds of three equal shares (states 4 and 5)."""
    from generate_music.grammar import OPEN, track_grammar
    from generate_music.transitions import start_thresholds
    from mgea.decoder import RowSchedule
    vocab = synth.decoder_vocab(300, with_eos=True)
    g = track_grammar(vocab)
    note0 = min(i for t, i in vocab.items() if t.startswith("[NOTE]"))
    note = lambda cls, j: note0 + 60 * cls + j   # START class cls (60 notes each)
    forced = [note(0, 3), note(0, 7), note(1, 2), note(2, 5), note(3, 1), note(4, 9), vocab["[INSTRUMENT] Flute"],
              note(0, 11), note(1, 4), note(1, 8), note(2, 6), note(3, 3), note(4, 2), note(4, 5)]
    sc = RowSchedule(tuple(start_thresholds(g, [1, 1, 1])), 1)
    variants = [[64, 79, 40, 275, 152], [83, 235, 287, 89, 269], [230, 238, 158, 273, 45]]   # transitions_util.ROWS[0]
    return g, OPEN, forced, sc, variants


def test_grammar_state_key_follows_the_start_of_the_last_note():
    from mgea.decoder import RowSampling
    g, start, forced, sc, variants = grammar_case()
    _, want, segs = tu.oracle_scheduled(tu.oracle(), variants, sc, len(forced), forced, grammar=g, start_state=start)
    _, plain, _ = tu.oracle_scheduled(tu.oracle(), variants, sc, len(forced), forced, grammar=g, start_state=start, splice=False)
    # the host model: OPEN and classes 0, 1 are segment 0, class 2 is 1, classes 3, 4 are 2; the new track falls back to 0
    assert segs == [0, 0, 0, 0, 1, 2, 2, 0, 0, 0, 0, 1, 2, 2]
    eng = make(max_batch=2)
    eng.set_grammar(g)
    rows = [RowSampling(top_k=1, grammar_state=start), RowSampling(top_k=1)]
    for n in (4, 5, 6, 8, 12, len(forced)):
        res = eng.generate_scheduled([variants, [2, 9]], rows, [sc, None], n, scored=True, force_ids=[forced[:n], None])
        assert res.ids[0].cpu().tolist() == forced[:n] and eng.id_errors(raise_error=False) == 0
        assert eng.segments().cpu().tolist() == [segs[n - 1], 0], f"after {n} steps"
        assert eng.schedule_info()["switches"] == sum(1 for a, b in zip([0] + segs[:n - 1], segs[:n]) if a != b)
    d = float((res.logprobs[0].cpu().double() - want).abs().max())
    # power, from the oracle alone: at every step the row spends outside segment 0 the splice moves the value by 10 bounds or more
    off = min(float(abs(want[i] - plain[i])) for i, sg in enumerate(segs) if sg > 0)
    print(f"[transitions] grammar key: |logprob - spliced oracle| {d:.2e} (bound {ORACLE_TOL:.1e}; the splice moves the switched steps by >= {off:.3f})")
    assert off >= 10 * ORACLE_TOL and d <= ORACLE_TOL
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 4. compositions
def test_windowed_run_switches_after_two_evictions():
    from mgea.decoder import RowSampling, RowSchedule
    n_steps, max_ctx = 330, 192   # P = 3 pages: a 5-token prompt evicts at steps 186 and 250
    first, variant = [1, 5, 9, 20, 21], [1, 6, 11, 20, 21]
    eng = make(max_batch=2, max_ctx=max_ctx)
    eng.set_window(1, None, max_steps=n_steps)
    rows = [RowSampling(1.0, 20, seed=5), RowSampling(1.0, 20, seed=6)]
    at = 260
    assert eng.window.evictions(len(first), at) == 2
    got = eng.generate_scheduled([[first, variant], [4, 8, 15]], rows, [RowSchedule((at,)), None], n_steps, scored=True)
    assert eng.window_evictions() == [eng.window.evictions(5, n_steps - 1), eng.window.evictions(3, n_steps - 1)]
    assert eng.schedule_info() == dict(scheduled_steps=n_steps, switches=1) and eng.segments().cpu().tolist() == [1, 0]
    stay = eng.generate_scored([first, [4, 8, 15]], rows, n_steps)
    assert torch.equal(got.ids[:, :at].cpu(), stay.ids[:, :at].cpu()) and torch.equal(got.logprobs[:, :at].cpu(), stay.logprobs[:, :at].cpu())
    assert torch.equal(got.ids[1].cpu(), stay.ids[1].cpu())
    assert not torch.equal(got.logprobs[0, at:].cpu(), stay.logprobs[0, at:].cpu()), "the switch behind two evictions changed nothing"
    eng.close()


def test_guided_pair_whose_conditional_row_switches():
    from mgea.decoder import RowSampling, RowSchedule
    first, variant, neg = [1, 5, 9, 20, 21], [1, 6, 11, 20, 21], [1, 20, 21]
    eng = make(max_batch=4)
    rows = [RowSampling(1.0, 20, seed=3), RowSampling(1.0, 20, seed=4)]
    n = 16
    got = eng.generate_scheduled([[first, variant], [3, 7, 20]], rows, [RowSchedule((0,)), None], n, scored=True,
                                 negative_prompts=[neg, None], guidance_scale=2.0)
    assert eng.guidance_info() == dict(pairs=1, guided_steps=n) and eng.schedule_info() == dict(scheduled_steps=n, switches=1)
    assert eng.segments().cpu().tolist() == [1, 0, 0]   # the shadow row (behind the callers' rows) has one segment
    want = eng.generate_guided([variant, [3, 7, 20]], [neg, None], rows, 2.0, n, scored=True, all_rows=True)
    assert torch.equal(got.ids.cpu(), want.ids[:2].cpu()) and torch.equal(got.logprobs.cpu(), want.logprobs[:2].cpu())
    assert torch.equal(want.ids[2].cpu(), want.ids[0].cpu())   # and the shadow's ids are the conditional row's
    stay = eng.generate_guided([first, [3, 7, 20]], [neg, None], rows, 2.0, n, scored=True)
    assert not torch.equal(got.logprobs[0].cpu(), stay.logprobs[0].cpu())
    with pytest.raises(ValueError, match="never capped"):
        eng.generate_scheduled([[first, variant]], rows[:1], [RowSchedule((0,))], eng.max_ctx, negative_prompts=[neg])
    eng.close()


def test_penalty_bias_and_grammar_rows_in_one_scheduled_batch():
    from mgea.decoder import RowSampling, RowSchedule, TokenGrammar
    eng = make(max_batch=4)
    eng.set_grammar(TokenGrammar(np.arange(eng.vocab) % 2, np.array([[1, -1], [-1, 0]])))   # even and odd ids alternate
    bias = (np.random.default_rng(5).standard_normal(eng.vocab) * 2).astype(np.float32)
    first, variant = [1, 5, 9, 20, 21], [1, 6, 11, 20, 21]
    rows = [RowSampling(1.0, 20, None, 1.3, seed=7), RowSampling(1.0, 20, seed=8, logit_bias=bias, min_new_tokens=3),
            RowSampling(1.0, 20, None, 1.2, seed=9, grammar_state=0)]
    n = 14
    prompts0 = [first, [3, 7, 20], first]
    segs = [[first, variant], [[3, 7, 20], [4, 8, 20]], [first, variant]]
    got = eng.generate_scheduled(segs, rows, [RowSchedule((6,)), RowSchedule((0,)), RowSchedule((1,), 1)], n, scored=True)
    # row 2's key is its grammar state, which alternates: it goes to and fro at every step after the first (13 switches)
    assert eng.schedule_info() == dict(scheduled_steps=n, switches=1 + 1 + 13) and eng.segments().cpu().tolist() == [1, 1, 1]
    pres = eng.presence().cpu()
    stay = eng.generate_scored(prompts0, rows, n)
    assert torch.equal(got.ids[0, :6].cpu(), stay.ids[0, :6].cpu()) and torch.equal(got.logprobs[0, :6].cpu(), stay.logprobs[0, :6].cpu())
    assert not torch.equal(got.logprobs.cpu(), stay.logprobs.cpu())
    ids2 = [int(v) for v in got.ids[2].cpu().tolist()]
    assert all(i % 2 == t % 2 for t, i in enumerate(ids2)), "the grammar row left its grammar"
    # the penalty set stays the FIRST prompt plus the generated ids: the scheduled run's bitmap of row 0 holds 5 and 9, not 6 and 11
    seen = set(pres[0].nonzero().flatten().tolist())
    assert seen == set(first) | {int(v) for v in got.ids[0].cpu().tolist()}
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. graphs, refusals, the app
def test_scheduled_graphs_are_reused_and_leave_the_unscheduled_ones_alone():
    from mgea.decoder import RowSampling, RowSchedule
    first, variant, other = [1, 5, 9, 20, 21], [1, 6, 11, 20, 21], [3, 7, 20]
    rows = [RowSampling(1.0, 20, seed=7), RowSampling(1.0, 20, seed=8)]
    eng, fresh = make(), make()
    n = 12
    before = eng.generate_rows([first, other], rows, n).cpu()
    eng.generate_rows([first, other], rows, 1)
    plain_nodes, unscheduled = eng.stats()["graph_nodes"], eng.stats()["graph_instantiates"]
    a = eng.generate_scheduled([[first, variant], other], rows, [RowSchedule((4,)), None], n).cpu()
    inst = eng.stats()["graph_instantiates"]
    assert inst > unscheduled, "the scheduled steps are graphs of their own"
    eng.generate_scheduled([[first, variant], other], rows, [RowSchedule((4,)), None], 1)
    assert eng.stats()["graph_nodes"] == plain_nodes + 1, "a scheduled step is the unscheduled one and ONE more launch"
    inst = eng.stats()["graph_instantiates"]
    b = eng.generate_scheduled([[first, variant], [other, [4, 8, 20]]], rows, [RowSchedule((9,)), RowSchedule((2,))], n).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "other thresholds and other scheduled rows captured a new graph"
    c = eng.generate_scheduled([[first, variant, [1, 8, 17, 20, 21]], other], rows, [RowSchedule((2, 5)), None], n).cpu()   # a bigger store
    assert eng.stats()["graph_instantiates"] == inst + 2, "a regrown store drops the scheduled graphs: the 1-step and the 8-step one again"
    inst = eng.stats()["graph_instantiates"]
    assert torch.equal(eng.generate_scheduled([[first, variant], other], rows, [RowSchedule((4,)), None], n).cpu(), a)
    assert eng.stats()["graph_instantiates"] == inst, "a smaller store / other thresholds captured a new scheduled graph"
    assert torch.equal(a[:, :4], before[:, :4]) and not torch.equal(a[0], before[0]) and not torch.equal(a[0], b[0]) and not torch.equal(a[0], c[0])
    after = eng.generate_rows([first, other], rows, n).cpu()
    assert eng.stats()["graph_instantiates"] == inst and eng.schedule_info() == dict(scheduled_steps=0, switches=0)
    eng.generate_rows([first, other], rows, 1)
    assert eng.stats()["graph_nodes"] == plain_nodes, "an unscheduled call after a scheduled one has the node count it had"
    want = fresh.generate_rows([first, other], rows, n).cpu()
    assert torch.equal(before, want) and torch.equal(after, want), "an unscheduled call next to a scheduled one drew other ids"
    # a call in which no row has more than one segment IS the existing call
    assert torch.equal(eng.generate_scheduled([first, other], rows, None, n).cpu(), want) and eng.stats()["graph_instantiates"] == inst
    with pytest.raises(RuntimeError, match="not scheduled"):
        eng.segments()
    eng.close()
    fresh.close()


def raw_scheduled(eng, ids, rows, sched, n_seg_max, n_steps, starts=None, guide=None):
    """mgea_decoder_generate_rows_scheduled itself on prompt ids [n_seg_max][B][Tp]; returns (status, message)"""
    from mgea import _lib
    from mgea.decoder import pack_rows
    ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    B, Tp = ids.shape[1:]
    out = torch.full((B, max(n_steps, 1)), -7, dtype=torch.int32, device="cuda")
    recs = pack_rows(rows, eng.vocab, n_steps)
    sarr = None
    if sched is not None:
        sarr = (_lib.RowSchedule * B)()
        for b, (n, key, th, res) in enumerate(sched):
            sarr[b].n_segments, sarr[b].key, sarr[b].reserved = n, key, res
            for s, t in enumerate(th):
                sarr[b].threshold[s] = t
    garr = None if guide is None else (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in guide])
    st = None if starts is None else (C.c_int32 * B)(*starts)
    with eng._on_stream():
        rc = eng.lib.mgea_decoder_generate_rows_scheduled(eng.h, _lib.ptr(ids), None, B, Tp, n_steps, recs, None, st, garr, sarr, n_seg_max,
                                                          None, _lib.ptr(out), None, None, eng._sp())
    torch.cuda.synchronize()
    return rc, _lib.last_error(), out.cpu()


def test_refusals_launch_nothing():
    from mgea import _lib
    from mgea.decoder import DecoderEngine, RowSampling
    eng = make(max_batch=3)
    rows = [RowSampling(1.0, 20, seed=3) for _ in range(2)]
    two = [[[5, 6, 7], [8, 9, 10]], [[5, 9, 7], [8, 9, 10]]]
    plain = (1, 0, (), 0)
    replays = eng.stats()["graph_instantiates"]
    for sched, n_seg, kw, code, who in (
            ([(0, 0, (), 0), plain], 2, {}, _lib.EINVAL, "row 0: n_segments 0"), ([(9, 0, (), 0), plain], 2, {}, _lib.EINVAL, "row 0: n_segments 9"),
            ([plain, (2, 0, (4,), 0)], 1, {}, _lib.EINVAL, "row 1: n_segments 2 exceeds n_seg_max 1"),
            ([(2, 0, (4,), 0), plain], 9, {}, _lib.EINVAL, "n_seg_max 9"), ([(2, 0, (4,), 0), plain], 0, {}, _lib.EINVAL, "n_seg_max 0"),
            ([(3, 0, (5, 4), 0), plain], 2, {}, _lib.EINVAL, "row 0: n_segments 3 exceeds"),
            ([plain, (2, 0, (-1,), 0)], 2, {}, _lib.EINVAL, "row 1: threshold"), ([plain, (2, 2, (1,), 0)], 2, {}, _lib.EINVAL, "row 1: key 2"),
            ([plain, (2, 0, (1,), 5)], 2, {}, _lib.EINVAL, "row 1: reserved"),
            ([(2, 1, (1,), 0), plain], 2, {}, _lib.EINVAL, "row 0: key 1 (grammar state) but no grammar"),
            ([plain, (2, 0, (1,), 0)], 2, dict(guide=[(1, 1.5), (-1, 0.0)]), _lib.EINVAL, "row 1 is a guidance shadow row"),
            (None, 2, {}, _lib.EINVAL, "no schedules")):
        rc, msg, out = raw_scheduled(eng, two[:n_seg] if 1 <= n_seg <= 2 else two, rows, sched, n_seg, 4, **kw)
        assert rc == code and who in msg, (sched, rc, msg)
        assert int((out != -7).sum()) == 0, "a refused call wrote ids"
    three = [[[5, 6, 7], [8, 9, 10]]] * 3
    rc, msg, _ = raw_scheduled(eng, three, rows, [(3, 0, (5, 4), 0), plain], 3, 4)
    assert rc == _lib.EINVAL and "row 0: thresholds not ascending" in msg
    wide = [[list(range(1, 66))] * 2] * 2
    big = make(max_batch=2, max_ctx=128)
    rc, msg, _ = raw_scheduled(big, wide, rows, [(2, 0, (1,), 0), plain], 2, 4)
    assert rc == _lib.ECAPACITY and "one page" in msg
    big.close()
    from generate_music.grammar import track_grammar
    eng.set_grammar(track_grammar(synth.decoder_vocab(eng.vocab, with_eos=True)))
    rc, msg, _ = raw_scheduled(eng, two, rows, [(2, 1, (3,), 0), plain], 2, 4, starts=[-1, -1])
    assert rc == _lib.EINVAL and "row 0: key 1 (grammar state) on a row without a start state" in msg
    assert eng.stats()["graph_instantiates"] == replays and eng.schedule_info() == dict(scheduled_steps=0, switches=0)
    rc, msg, out = raw_scheduled(eng, two, rows, [(2, 1, (3,), 0), plain], 2, 4, starts=[1, -1])
    assert rc == 0 and int(out.min()) >= 0, msg
    eng.close()
    sd, n_head, _ = tu.model("tiny")
    twin = DecoderEngine(sd, n_head=n_head, max_batch=2, max_ctx=32, block_mode="postln_relu")   # the no-cache twin has no pages to swap
    rc, msg, _ = raw_scheduled(twin, two, rows, [(2, 0, (1,), 0), plain], 2, 4)
    assert rc == _lib.EINVAL and "KV-cache block mode" in msg
    twin.close()


def test_transition_endpoint(golden, monkeypatch):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_transition_app
    from emotion_analysis import EATS, inference
    from generate_music.midi import note_re

    g = golden("decoder_tiny8h")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    labels = {"i lost my keys": "sadness", "then i found them": "joy", "now i am calm": "relief"}
    monkeypatch.setattr(inference, "predict", lambda text: next(v for k, v in labels.items() if k in text.lower()))   # the stubbed classifier
    monkeypatch.setattr(gen, "_draw_seed", lambda: 1234)
    app = create_transition_app(model, seq_len=40, temperature=1.0, top_k=20)
    served = []
    app.state.on_tokens = served.append
    client = TestClient(app)
    text = "I lost my keys. Then I found them! Now I am calm."
    kw = {"data": {"prompt": text}} if app.state.prompt_in == "form" else {"params": {"prompt": text}}
    random.seed(11)
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and r.content[:4] == b"MThd"
    assert r.headers["x-emotions"] == "sadness,joy,relief" and r.headers["x-segments"] == "3" and r.headers["x-emotion"] == "sadness"
    assert r.headers["x-grammar"] == "tracks"
    info = model._need().schedule_info()
    assert 0 < info["scheduled_steps"] <= 40 - int(r.headers["x-prompt-tokens"])
    tokens = served[0]
    n_prompt = int(r.headers["x-prompt-tokens"])
    random.seed(11)
    first = EATS.get_music_params("sadness")
    assert tokens[1] == gen.closest_bpm_token(first["bpm"]) and tokens[2] == gen.normalize_key_signature(first["key"])
    assert len(tokens) == int(r.headers["x-generated-tokens"]) and any(note_re.match(t) for t in tokens[n_prompt:])
    with pytest.raises(ValueError, match="guidance_scale"):
        create_transition_app(model, seq_len=40, guidance_scale=-1.0)
