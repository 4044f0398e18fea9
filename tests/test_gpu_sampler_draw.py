"""The sampler's draw (csrc/sampler.hip, the second half of sample_kernel) on the MI355X against the host restatement of
tests/sampler_draw_util.py: a Philox4x32-10 in Python integers, the counter {stream, step, step >> 32, 0x6d676561} under the key
(seed low, seed high), u = (word 0 >> 8) * 2^-24, and a float64 CDF in the kernel's thread-major order.  tests/test_sampler_draw_host.py
proves the restatement's premises on the CPU (the Random123 known answers among them) and the input condition of the tolerance family.

Every case is ONE logits row repeated over the rows of a launch with different counters: thousands of draws from a handful of
launches, one float64 CDF per case.

* Exact family (assertion ==): n kept entries at logit 0, n a power of two, everything else -inf.  exp(0) = 1, every partial sum is an
  integer below 2^24 and u * n is exact, so the drawn id MUST be the kept id at index floor(u * n) of the CDF order.  Each case is also
  run on counters whose u sits exactly on a thread boundary (sampler_draw_util.BOUNDARY_STREAMS).
* Tolerance family: rows robust() admits (tests/truncation_util.py), reference p from DecoderRef.masked_probs / truncated_probs in
  float64; every drawn id must be in admissible(p, u, 2e-5).  2e-5 is the project's fp32 row-operation bound; what it has to cover, in
  units of the normalised CDF:
      the kernel's partial sum in front of an id: at most 56 (registers) + 6 (lane scan) + 4 (wave totals) = 66 fp32 additions, each
          rounding a value <= total by at most 2^-24 of it                                                     66 * 6e-8 = 4e-6
      the total the target u * total is formed from: the same 66 additions                                                 4e-6
      x / temperature (half an ulp of |x| <= 32 in the exponent) and __expf: a relative 2e-6 on every term, at most twice that on
          a normalised partial sum                                                                                          4e-6
  together 1.2e-5 in the worst case, under the bound.  The host test shows that at this delta at least 85 % of every case's draws
  admit exactly ONE id, so the assertion is close to an equality.

Observed on an MI355X, the largest distance between u and the drawn id's float64 interval (bound 2e-5):
    the tolerance family, 31 cases x 256 draws                          0     (every u lay inside the float64 interval of its id)
    every entry point at V = 8324 and 14336, 2 x 16 x 256 draws         0
    the engine's generation replayed, 4 rows x 24 steps                 4.2e-9
The exact family has no distance: 10 cases x (256 + 6) draws, the entry points' 2 x 16 x 256 and the counter-word draws are equal."""
import numpy as np
import pytest
import torch

import sampler_draw_util as D
import step_tail_util as U
from mgea import synth

pytestmark = pytest.mark.gpu
B = D.B_DRAWS


def tile(x, n):
    return torch.from_numpy(np.ascontiguousarray(x)).repeat(n, 1).cuda()


def records(counters, temp=1.0, k=0, top_p=None, pen=None, **kw):
    from mgea.decoder import RowSampling
    return [RowSampling(temp, k, top_p, pen, seed=seed, stream=stream, **kw) for seed, stream in counters]


def us_of(counters, step):
    return np.asarray([D.draw_u(seed, stream, step) for seed, stream in counters])


def check_exact(ids, kept, us, what):
    got, want = np.asarray(ids.cpu(), np.int64), D.exact_expected(kept, us)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} draws off the rule, first rows {bad[:6].tolist()}: got {got[bad[:6]].tolist()} "
                           f"want {want[bad[:6]].tolist()} at u * n = {(us[bad[:6]] * len(kept)).tolist()}")


def check_admissible(ids, p, us, what):
    got = np.asarray(ids.cpu(), np.int64)
    d = D.distance(p, us, got)
    print(f"OBSERVED {what}: largest distance between u and the drawn id's fp64 interval {float(d.max()):.3e} "
          f"(draws outside their interval: {int((d > 0).sum())} of {len(d)})")
    bad = np.flatnonzero(~(d <= D.DELTA))
    if bad.size:
        r = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {len(d)} drawn ids are not admissible at delta {D.DELTA}; row {r}: u = {us[r]!r}, drew "
                             f"{int(got[r])} ({d[r]:.3e} away), admissible {D.admissible(p, us[r], D.DELTA).tolist()}")
    return float(d.max())


# ---------------------------------------------------------------------------------------------------------- 1. the exact family
@pytest.mark.parametrize("name", list(D.EXACT_CASES))
def test_exact_family(name):
    from mgea import ops
    x, kept, k = D.exact_case(name)
    index = list(D.EXACT_CASES).index(name)
    for which, (counters, step) in (("counters", D.counters(index, B)), ("thread boundaries", D.boundary_counters())):
        ids = ops.sample_rows(tile(x, len(counters)), records(counters, 1.0, k), step=step)
        check_exact(ids, kept, us_of(counters, step), f"{name} ({which}, step {step})")


# ---------------------------------------------------------------------------------------------------------- 2. the tolerance family
@pytest.mark.parametrize("case", D.TOLERANCE_CASES, ids=D.case_id)
def test_tolerance_family(case):
    from mgea import ops
    from mgea.decoder import Truncation
    x, p, (temp, k, top_p, st) = D.tolerance_case(case)
    counters, step = D.counters(D.TOLERANCE_CASES.index(case), B)
    dev = tile(x, B)
    if st:
        ids = ops.sample_rows_truncated(dev, records(counters, temp, k, top_p, truncation=Truncation(**st)), step=step)
    else:
        ids = ops.sample_rows(dev, records(counters, temp, k, top_p), step=step)
    check_admissible(ids, p, us_of(counters, step), D.case_id(case))


# ---------------------------------------------------------------------------------------------------------- 3. every instantiation
def entry_points(V):
    """name -> call(dev, temp, k, top_p, seed, step) -> (ids, choice_logprobs or None): one per <PENALTY, BIAS, ScoreArgs, GrammarArgs,
    TruncArgs> instantiation of sample_kernel (14 of them at either register width), each with NEUTRAL settings where its form needs
    some: a penalty over an empty presence set, a zero bias, a one-state grammar that allows every id, a Truncation with nothing on."""
    from mgea import ops
    from mgea.decoder import RowSampling, TokenGrammar, Truncation
    zero = torch.zeros(V, device="cuda")
    gram = TokenGrammar(np.zeros(V, np.int32), np.zeros((1, 1), np.int32))
    off = Truncation()

    def rows(temp, k, top_p, seed, pen=None, bias=None):
        return [RowSampling(temp, k, top_p, pen, seed=seed, logit_bias=bias) for _ in range(B)]      # stream None = the row's index

    def scored(out):
        return out[0], out[2]

    e = {}
    e["sample"] = lambda dev, t, k, p, seed, step: (ops.sample(dev, t, k, p, seed=seed, step=step), None)
    e["sample penalized"] = lambda dev, t, k, p, seed, step: (ops.sample(dev, t, k, p, seed=seed, step=step, repetition_penalty=1.3), None)
    for name, pen, bias in (("", None, None), (" +presence", 1.3, None), (" +bias", None, zero), (" +bias +presence", 1.3, zero)):
        e["sample_rows" + name] = lambda dev, t, k, p, seed, step, pen=pen, bias=bias: \
            (ops.sample_rows(dev, rows(t, k, p, seed, pen, bias), step=step), None)
        e["sample_rows_scored" + name] = lambda dev, t, k, p, seed, step, pen=pen, bias=bias: \
            scored(ops.sample_rows_scored(dev, rows(t, k, p, seed, pen, bias), step=step))
    e["sample_rows_grammar"] = lambda dev, t, k, p, seed, step: (ops.sample_rows_grammar(dev, rows(t, k, p, seed), gram, [0] * B, step=step)[0], None)
    e["grammar scored"] = lambda dev, t, k, p, seed, step: \
        scored(ops.sample_rows_truncated(dev, rows(t, k, p, seed), step=step, scored=True, grammar=gram, states=[0] * B))
    e["sample_rows_truncated"] = lambda dev, t, k, p, seed, step: (ops.sample_rows_truncated(dev, rows(t, k, p, seed), off, step=step), None)
    e["truncated scored"] = lambda dev, t, k, p, seed, step: scored(ops.sample_rows_truncated(dev, rows(t, k, p, seed), off, step=step, scored=True))
    e["truncated grammar"] = lambda dev, t, k, p, seed, step: \
        (ops.sample_rows_truncated(dev, rows(t, k, p, seed), off, step=step, grammar=gram, states=[0] * B)[0], None)
    e["truncated grammar scored"] = lambda dev, t, k, p, seed, step: \
        scored(ops.sample_rows_truncated(dev, rows(t, k, p, seed), off, step=step, scored=True, grammar=gram, states=[0] * B))
    return e


@pytest.mark.parametrize("V", sorted(D.ENTRY_EXACT))
def test_every_instantiation_draws_by_the_rule(V):
    """one exact and one tolerance case through every entry point that selects another sample_kernel; the scored forms' choice
    log-probability of the drawn id is log p[id] within the op-level bound of tests/test_gpu_logprobs.py"""
    from test_gpu_logprobs import OP_TOL
    counters, step = D.entry_counters(B)
    seed = counters[0][0]
    us = us_of(counters, step)
    x0, kept, k0 = D.exact_case(D.ENTRY_EXACT[V])
    x1, p1, (temp, k1, top_p, st) = D.tolerance_case(D.ENTRY_TOLERANCE[V])
    assert not st and len(x0) == V and len(x1) == V
    dev0, dev1 = tile(x0, B), tile(x1, B)
    n_scored = 0
    for name, call in entry_points(V).items():
        ids, ch = call(dev0, 1.0, k0, None, seed, step)
        check_exact(ids, kept, us, f"V={V} {name}: exact case")
        if ch is not None:
            assert float((ch.cpu().double() + np.log(len(kept))).abs().max()) <= OP_TOL, f"V={V} {name}: choice logprob of a 1 / n row"
        ids, ch = call(dev1, temp, k1, top_p, seed, step)
        check_admissible(ids, p1, us, f"V={V} {name}: tolerance case")
        if ch is not None:
            n_scored += 1
            want = np.log(p1[np.asarray(ids.cpu(), np.int64)])
            d = float(np.abs(ch.cpu().double().numpy() - want).max())
            assert d <= OP_TOL, f"V={V} {name}: choice logprob of the drawn id off log p[id] by {d:.2e}"
    assert n_scored == 7


# ---------------------------------------------------------------------------------------------------------- 4. the counter's words
def test_counter_and_key_words():
    from mgea import ops
    x, kept, _ = D.exact_case("d_flat_8192")        # 13 bits of u decide the id: two different draws collide once in 8192
    n = 64
    dev = tile(x, n)
    seed = 0x0BADC0DE00000011
    # a call without records: row b draws from stream b; the step's high half is word 2
    want = {}
    for step in (3, 2 ** 32 + 3):
        us = us_of([(seed, b) for b in range(n)], step)
        want[step] = D.exact_expected(kept, us)
        check_exact(ops.sample(dev, 1.0, 0, None, seed=seed, step=step), kept, us, f"ops.sample, step {step}: stream b, word 2 = step >> 32")
    assert int((want[3] != want[2 ** 32 + 3]).sum()) >= n - 2, "the two steps must draw differently for the check to mean anything"
    # records: streams up to 2^32 - 1, seeds on either side of 2^32, two seeds that are each other's halves swapped
    a, b = 0x0000000500000007, 0x0000000700000005
    counters = [(seed, 2 ** 32 - 1), (seed, 2 ** 32 - 2), (seed, 2 ** 31), (seed, 0), (seed & 0xFFFFFFFF, 5), (seed, 5), (seed >> 32, 5),
                (a, 9), (b, 9), (a << 8, 9), (2 ** 64 - 1, 2 ** 32 - 1), (2 ** 63, 1), (1, 2 ** 31 + 1)]
    counters += [(s, 77 - i) for i, s in enumerate(range(2 ** 32 - 3, 2 ** 32 + 3))]
    for step in (0, 7, 2 ** 32 + 3):
        us = us_of(counters, step)
        assert len(set(D.exact_expected(kept, us).tolist())) >= len(counters) - 1
        check_exact(ops.sample_rows(dev[:len(counters)], records(counters), step=step), kept, us, f"ops.sample_rows, step {step}")


def test_fused_tail_draws_from_the_rows_own_step():
    """ops.step_tail kind 4 (the sampler with its fused tail): word 1 of row b's counter is row_step[b], a different one on every row,
    whatever the host's step is; the state the tail leaves is the rule's for the drawn ids"""
    from mgea import _lib, ops
    from mgea.decoder import RowSampling
    from test_gpu_step_tail import VOCAB, Buf, Embed, State, i32
    n = 64
    sc = U.scenarios(n, True)
    sc["step"] = np.asarray([(5 * j) % 67 for j in range(n)], np.int64)      # distinct, on both sides of ids_out's width
    sc["max_new"] = np.zeros(n, np.int64)
    assert len(set(sc["step"].tolist())) == n
    kept_ids = list(range(7, 39))                   # 32 of the 50 ids, the scenarios' EOS (2) not among them
    x = D.exact_row(VOCAB, kept_ids)
    order = D.cdf_order(VOCAB)
    kept = order[np.isin(order, kept_ids)]
    counters = [(0x5EED000000000000 + 3 * j if j % 2 else 40 + j, (2654435761 * (j + 1)) & 0xFFFFFFFF) for j in range(n)]
    us = np.asarray([D.draw_u(seed, stream, int(sc["step"][j])) for j, (seed, stream) in enumerate(counters)])
    sc["tok"] = D.exact_expected(kept, us)
    ex = U.expected_state(sc, True)
    rows = [RowSampling(1.0, 0, None, None, int(sc["eos"][j]), 0, seed, stream) for j, (seed, stream) in enumerate(counters)]
    st, sampled, em = State(sc), Buf.poison(n, torch.int32), Embed(n, 128)
    ops.step_tail(_lib.TAIL_SAMPLE, n, st.args(), rows=rows, ctx_cap=[int(c) for c in sc["cap"]], sampled=sampled.t,
                  sampler=dict(logits=tile(x, n).reshape(-1)), **em.args())
    check_exact(sampled.cpu(), kept, us, "fused tail: word 1 is the row's own step")
    sampled.pads_intact("fused tail: sampled")
    st.check(ex, "fused tail")
    em.check(ex["fed"], ex["next_len"], "fused tail")
    # the same rows at the host's step 0 draw something else
    assert int((D.exact_expected(kept, us_of(counters, 0)) != sc["tok"]).sum()) >= n - 8


# ---------------------------------------------------------------------------------------------------------- 5. the engine
def test_generation_step_t_draws_from_counter_word_t(golden):
    """step t of a generation is word 1 = t, starting at 0: every id generate_rows produced is admissible for the logits a replay
    of the same ids yields, under counter {stream_b, t, 0, const} and key seed_b"""
    from mgea.decoder import DecoderEngine, RowSampling
    from oracle.decoder_ref import DecoderRef
    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(v) for v in g["cfg"])
    eng = DecoderEngine(synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer), n_head=n_head, max_batch=8, max_ctx=seq_len)
    rng = np.random.default_rng(97)
    prompts = [[int(v) for v in rng.integers(0, vocab, int(rng.integers(4, 10)))] for _ in range(4)]
    n_steps = 24
    rows = [RowSampling(1.0, 0, seed=0x7000000000000001, stream=2 ** 32 - 1), RowSampling(0.9, 50, seed=5, stream=0),
            RowSampling(1.1, 0, 0.95, seed=2 ** 32 + 5, stream=3), RowSampling(0.8, 40, 0.9, seed=0x0000000500000000, stream=2 ** 31)]
    out = eng.generate_rows(prompts, rows, n_steps).cpu()
    assert int(out.min()) >= 0
    Tp = max(len(q) for q in prompts)
    idx = torch.zeros(4, Tp, dtype=torch.long)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
    eng.reset_and_prefill(idx, torch.tensor([len(q) for q in prompts]), want_logits=False, max_len=Tp + n_steps)
    fed = torch.tensor([q[-1] for q in prompts], dtype=torch.int32)
    worst = 0.0
    for t in range(n_steps):
        _, lg = eng.step(fed, eng.sampler(1.0, 1), want_logits=True)
        lg = lg.cpu().double()
        for b, r in enumerate(rows):
            p = DecoderRef.masked_probs(lg[b:b + 1], r.temperature, r.top_k or None, r.top_p)[0].numpy()
            u = D.draw_u(r.seed, r.stream, t)
            d = float(D.distance(p, [u], [int(out[b, t])])[0])
            worst = max(worst, d)
            assert d <= D.DELTA, (f"row {b} step {t}: id {int(out[b, t])} is {d:.3e} from u = {u!r} under counter word 1 = {t}; "
                                  f"admissible {D.admissible(p, u, D.DELTA).tolist()}")
        fed = out[:, t].to(torch.int32)
    print(f"OBSERVED engine: largest distance between u and the drawn id's fp64 interval {worst:.3e}")
    eng.close()
