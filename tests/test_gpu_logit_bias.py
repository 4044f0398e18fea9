"""Per-row logit bias and min_new_tokens on the MI355X: the BIAS sampler against the fp32 restatement, biased greedy generation
against the oracle, bans that hold over sampled generations, min_new_tokens, the sampled draw replayed step by step, every launch
form of generate_biased(), graph reuse, the unbiased paths left as they were, the fp16 engine, and the constrained endpoint end to end.

Tolerances are those of tests/test_gpu_repetition_penalty.py: probabilities atol 2e-6 / rtol 1e-4; a greedy generation may leave the
oracle's only where the oracle's own top-2 gap is below NEAR_TIE.

decoder_tiny has 64 positions, so its oracle comparison runs 52 steps (64 - 12, the longest prompt) instead of 100."""
import math
import random

import numpy as np
import pytest
import torch

from mgea import synth
from test_repetition_penalty_host import penalize

pytestmark = pytest.mark.gpu
NEAR_TIE = 1e-4
NINF = -math.inf
SETTINGS = ((None, None), (50, None), (None, 0.92), (50, 0.92), (1, None))   # (top_k, top_p) of the penalty test


def make(g, max_batch=8, max_ctx=None, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=max_batch, max_ctx=max_ctx or seq_len, **kw), sd, n_head


def rand_prompts(rng, B, vocab, lo, hi):
    return [list(rng.integers(0, vocab, int(rng.integers(lo, hi + 1)))) for _ in range(B)]


def make_bias(rng, kind, shape):
    """the issue's recipe: "finite" = N(0, 2); "ban70" = -inf with probability 0.7; "mixed" = finite, then -inf with probability 0.3"""
    if kind == "finite":
        return (rng.standard_normal(shape) * 2).astype(np.float32)
    if kind == "ban70":
        return np.where(rng.random(shape) < 0.7, NINF, 0.0).astype(np.float32)
    if kind == "mixed":
        b = (rng.standard_normal(shape) * 2).astype(np.float32)
        return np.where(rng.random(shape) < 0.3, NINF, b).astype(np.float32)
    raise KeyError(kind)


def ref_biased_greedy(ref, prompts, n_steps, bias=None, eos=None, min_new=None, penalty=None):
    """DecoderRef.forward per step, (penalize,) + bias, EOS banned while step < min_new, argmax (lowest id among equals).  bias
    [B, V] or None; eos / min_new: one per row or None.  Returns the generated ids [B][n_steps] (-1 after a row's EOS) and the
    processed top-2 gap of every (row, step)."""
    B = len(prompts)
    Tp = max(len(q) for q in prompts)
    idx = torch.zeros(B, Tp, dtype=torch.long)
    valid = torch.zeros(B, Tp, dtype=torch.bool)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
        valid[b, :len(q)] = True
    _, cache, cvalid = ref.forward(idx, None, None, valid)
    last = torch.tensor([q[-1] for q in prompts]).view(B, 1)
    seen = [set(q) for q in prompts]
    out, gaps = [[] for _ in range(B)], np.full((B, n_steps), np.inf)
    done = [False] * B
    for s in range(n_steps):
        logits, cache, cvalid = ref.forward(last, cache, cvalid, None)
        x = logits[:, -1, :].numpy().astype(np.float32)
        if penalty is not None:
            x = penalize(x, seen, penalty)
        if bias is not None:
            x = (x + bias).astype(np.float32)
        for b in range(B):
            if eos is not None and eos[b] >= 0 and min_new is not None and s < min_new[b]:
                x[b, eos[b]] = NINF
        nxt = x.argmax(1)
        srt = np.sort(x, 1)
        with np.errstate(invalid="ignore"):
            gaps[:, s] = np.where(np.isfinite(srt[:, -2]), srt[:, -1] - srt[:, -2], np.inf)
        for b in range(B):
            out[b].append(-1 if done[b] else int(nxt[b]))
            if not done[b]:
                seen[b].add(int(nxt[b]))
                done[b] = eos is not None and eos[b] >= 0 and int(nxt[b]) == eos[b]
        last = torch.from_numpy(nxt.astype(np.int64)).view(B, 1)
    return out, gaps


def exempted_rows(got, want, gaps, label):
    """rows that left the oracle's ids; each must have done so on an oracle near-tie"""
    n = 0
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            s = next(i for i in range(len(w)) if g[i] != w[i])
            assert gaps[b, s] < NEAR_TIE, f"{label}: row {b} diverged at step {s} (processed top-2 gap {gaps[b, s]:.3e})"
            print(f"[bias] {label}: row {b} differs at step {s} on a near-tie ({gaps[b, s]:.3e})")
            n += 1
    return n


# ---------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("V", [100, 8324, 14336])
def test_op_sample_biased_vs_restatement(V):
    from mgea import ops
    from mgea.decoder import RowSampling
    from oracle.decoder_ref import DecoderRef
    rng = np.random.default_rng(1000 + V)
    B = 4
    logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32))
    only10 = np.full((B, V), NINF, np.float32)
    for b in range(B):
        only10[b, rng.choice(V, 10, replace=False)] = 0.0
    combined = make_bias(rng, "mixed", (B, V))
    kinds = {"none": (None, None, None), "finite": (make_bias(rng, "finite", (B, V)), None, None),
             "ban70": (make_bias(rng, "ban70", (B, V)), None, None), "only10": (only10, None, None),
             "combined": (combined, rng.random((B, V)) < 0.2, 1.3)}
    dev = logits.cuda()
    for kname, (bias, mask, pen) in kinds.items():
        x = logits.numpy() if pen is None else penalize(logits.numpy(), mask, pen)
        x = torch.from_numpy(x if bias is None else (x + bias).astype(np.float32))
        pres = None if mask is None else torch.from_numpy(mask)
        for temp in (1.0, 0.7):
            for k, tp in SETTINGS:
                label = f"V={V} {kname} T={temp} k={k} top_p={tp}"
                want = DecoderRef.masked_probs(x, temp, min(k, V) if k else None, tp)
                assert bool(torch.isfinite(want).all()) and bool((want[torch.isinf(x)] == 0).all()), label
                # one [B, V] matrix through sample_biased(), and the same vectors in the rows' own records through sample_rows()
                ids, probs = ops.sample_biased(dev, temp, k, tp, seed=9, step=3, want_probs=True, repetition_penalty=pen, presence=pres,
                                               logit_bias=bias)
                rows = [RowSampling(temp, k, tp, pen, seed=9, logit_bias=None if bias is None else bias[b]) for b in range(B)]
                ids2, probs2 = ops.sample_rows(dev, rows, step=3, want_probs=True, presence=pres)
                if not (bias is None and k == 1):   # (sample() without records divides the greedy row by T; the records do not)
                    assert torch.equal(ids, ids2) and torch.equal(probs, probs2), label
                for i, p in ((ids, probs), (ids2, probs2)):
                    np.testing.assert_allclose(p.cpu().numpy(), want.numpy(), atol=2e-6, rtol=1e-4, err_msg=label)
                    assert bool((want.gather(1, i.cpu().long()[:, None]) > 0).all()), label + ": drew outside the kept set"
                    if bias is not None:
                        assert bool(np.isfinite(bias[np.arange(B), i.cpu().numpy()]).all()), label + ": drew a banned id"
                    if k == 1:
                        assert i.cpu().tolist() == x.numpy().argmax(1).tolist(), label


def test_op_sample_biased_exact_ties():
    from mgea import ops
    V = 300
    x = torch.full((4, V), -50.0)
    bias = np.zeros((4, V), np.float32)
    x[0, 10], x[0, 7] = 1.0, 2.0
    bias[0, 10] = 1.0                      # biased 1 + 1 == unbiased 2 at a LOWER id: 7 wins
    x[1, 7], x[1, 10] = 1.0, 2.0
    bias[1, 7] = 1.0                       # the biased entry is the lower id: 7 wins again
    x[2, 200], x[2, 100] = 4.0, 2.5
    bias[2, 200] = -1.5                    # 4 - 1.5 == 2.5 at a lower id: 100 wins
    x[3, 5], x[3, 6] = 3.0, 3.0
    bias[3, 5] = NINF                      # a banned maximum: 6
    assert ops.sample_biased(x.cuda(), 1.0, 1, None, logit_bias=bias).cpu().tolist() == [7, 7, 100, 6]
    assert ops.sample(x.cuda(), 1.0, 1, None).cpu().tolist() == [7, 10, 200, 5]
    # the k-th largest tied between biased and unbiased entries: exactly top_k kept, the tied ones by ascending id
    y = torch.full((1, V), -50.0)
    y[0, 250] = 5.0
    y[0, 20], y[0, 40], y[0, 60] = 2.0, 1.0, 2.0
    b = np.zeros((1, V), np.float32)
    b[0, 40] = 1.0                         # 20, 40, 60 all at 2.0
    _, p = ops.sample_biased(y.cuda(), 1.0, 3, None, want_probs=True, logit_bias=b)
    kept = torch.nonzero(p[0].cpu()).view(-1).tolist()
    assert kept == [20, 40, 250]
    # fewer admissible ids than top_k: the k-th largest is -inf, and what is kept of the banned ids weighs exactly 0
    b2 = np.full((1, V), NINF, np.float32)
    b2[0, [20, 250]] = 0.0
    ids, p = ops.sample_biased(y.cuda(), 1.0, 50, 0.92, want_probs=True, logit_bias=b2)
    from oracle.decoder_ref import DecoderRef
    want = DecoderRef.masked_probs(y + torch.from_numpy(b2), 1.0, 50, 0.92)
    assert torch.nonzero(want[0]).view(-1).tolist() == [250]          # p(250) = 0.953 reaches top_p alone
    np.testing.assert_allclose(p.cpu().numpy(), want.numpy(), atol=2e-6, rtol=1e-4)
    assert ids.cpu().tolist() == [250]
    _, p = ops.sample_biased(y.cuda(), 1.0, 50, None, want_probs=True, logit_bias=b2)
    want = DecoderRef.masked_probs(y + torch.from_numpy(b2), 1.0, 50, None)
    assert torch.nonzero(want[0]).view(-1).tolist() == [20, 250]
    np.testing.assert_allclose(p.cpu().numpy(), want.numpy(), atol=2e-6, rtol=1e-4)


def test_op_rows_without_a_bias_are_bitwise_the_old_op():
    from mgea import ops
    from mgea.decoder import RowSampling
    rng = np.random.default_rng(3)
    B, V = 6, 8324
    logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32)).cuda()
    mask = torch.from_numpy(rng.random((B, V)) < 0.1)
    bias = make_bias(rng, "mixed", V)
    for temp, k, tp, pen in ((1.0, 50, None, None), (0.8, None, 0.92, None), (1.0, 50, 0.92, 1.2), (1.3, None, None, None),
                             (1.0, 1, None, None), (0.7, 1, None, 1.4)):
        rows = [RowSampling(temp, k, tp, pen, seed=42, eos_id=11) for _ in range(B)]
        a_ids, a_p = ops.sample_rows(logits, rows, step=5, want_probs=True, presence=mask)
        # the BIAS kernel (row 5 has a bias), rows 0..4 without one; and a min_new_tokens that the step has passed
        rows_b = rows[:5] + [RowSampling(temp, k, tp, pen, seed=42, logit_bias=bias)]
        b_ids, b_p = ops.sample_rows(logits, rows_b, step=5, want_probs=True, presence=mask)
        assert torch.equal(a_ids[:5], b_ids[:5]) and torch.equal(a_p[:5], b_p[:5])
        c_ids, c_p = ops.sample_rows(logits, rows, step=5, want_probs=True, presence=mask, min_new_tokens=5)
        assert torch.equal(a_ids, c_ids) and torch.equal(a_p, c_p)
        # ... and one it has not: only the EOS entry goes
        d_ids, d_p = ops.sample_rows(logits, rows, step=4, want_probs=True, presence=mask, min_new_tokens=5)
        assert bool((d_p[:, 11] == 0).all()) and bool((d_ids != 11).all())


def test_device_bias_is_checked_with_one_reduction_and_check_false_skips_it():
    from mgea.decoder import RowSampling, pack_row_logits
    v = torch.zeros(100, device="cuda")
    v[3] = math.nan
    with pytest.raises(ValueError, match="row 1: .*NaN"):
        pack_row_logits([RowSampling(), RowSampling(logit_bias=v)], 100, "cuda")
    recs, keep = pack_row_logits([RowSampling(), RowSampling(logit_bias=v)], 100, "cuda", check=False)
    assert recs[1].bias_dev == v.data_ptr() and keep[0].data_ptr() == v.data_ptr()
    w = torch.full((100,), NINF, device="cuda")
    with pytest.raises(ValueError, match="row 0: .*bans every token"):
        pack_row_logits([RowSampling(logit_bias=w)], 100, "cuda")
    w[9] = 0.0
    pack_row_logits([RowSampling(logit_bias=w, eos_id=9)], 100, "cuda")
    with pytest.raises(ValueError, match="row 0: .*eos_id 9"):
        pack_row_logits([RowSampling(logit_bias=w, eos_id=9, min_new_tokens=2)], 100, "cuda")
    w[5] = math.inf
    with pytest.raises(ValueError, match=r"row 0: .*\+inf"):
        pack_row_logits([RowSampling(logit_bias=w)], 100, "cuda")


# ---------------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("tag", ["S", "tiny"])
def test_engine_biased_greedy_vs_oracle(golden, tag):
    from oracle.decoder_ref import DecoderRef
    g = golden("decoder_" + tag)
    eng, sd, n_head = make(g, max_batch=64)
    ref = DecoderRef(sd, n_head)
    V, L = eng.vocab, eng.seq_len
    n_steps = min(100, L - 12)
    changed = False
    for B in (1, 4, 64):
        rng = np.random.default_rng(53)
        prompts = [list(rng.integers(0, V, int(rng.integers(4, 13)))) for _ in range(B)]
        plain = eng.generate(prompts, n_steps, 1.0, 1).cpu().tolist()
        assert eng.stats()["biased_steps"] == 0
        for kind in ("finite", "ban70", "mixed"):
            bias = make_bias(rng, kind, (B, V))
            got = eng.generate_biased(prompts, n_steps, 1.0, 1, logit_bias=bias).cpu().tolist()
            assert eng.stats()["biased_steps"] == n_steps and eng.stats()["penalized_steps"] == 0
            want, gaps = ref_biased_greedy(ref, prompts, n_steps, bias)
            near = int((gaps < NEAR_TIE).any(axis=1).sum())
            n_ex = exempted_rows(got, want, gaps, f"{tag} B={B} {kind}")
            print(f"[bias] {tag} B={B} {kind}: min gap {gaps.min():.3e}, rows with a near-tie {near}, rows exempted {n_ex}")
            assert n_ex <= B // 16, f"{tag} B={B} {kind}: {n_ex} rows end on the near-tie exemption (cap {B // 16})"
            for b in range(B):
                assert all(np.isfinite(bias[b, i]) for i in got[b]), f"{tag} B={B} {kind}: row {b} produced a banned id"
            changed = changed or got != plain
    assert changed, "the bias never changed a greedy generation"


def test_bans_hold_over_sampled_generations(golden):
    from generate_music import constraints
    from generate_music.midi import note_name_to_number, note_re
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=64)
    V = eng.vocab
    rng = np.random.default_rng(59)
    prompts = rand_prompts(rng, 64, V, 4, 12)
    ban = make_bias(rng, "ban70", V)
    for kw in (dict(top_k=50), dict(top_k=0, top_p=0.92), dict(top_k=0)):
        out = eng.generate_biased(prompts, 200, 1.0, seed=7, logit_bias=ban, **kw).cpu().numpy()
        assert out.min() >= 0 and np.isfinite(ban[out]).all(), f"{kw}: a banned id was drawn"
        assert len({tuple(r) for r in out.tolist()}) > 1
    vocab = synth.decoder_vocab(V, with_eos=True)
    names = list(vocab)
    scale = constraints.scale_pitch_classes("E♭ Major")
    bias = constraints.logit_bias(vocab, key="E♭ Major")
    for kw in (dict(top_k=50), dict(top_k=0, top_p=0.92), dict(top_k=0)):
        out = eng.generate_biased(prompts, 200, 1.0, seed=8, logit_bias=torch.from_numpy(bias).cuda(), **kw).cpu().tolist()
        n_notes = 0
        for row in out:
            for i in row:
                tok = names[i]
                m = note_re.match(tok)
                assert m or tok.startswith("[INSTRUMENT]") or tok == "[END_SEQUENCE]", f"{kw}: control token {tok!r} after the prompt"
                if m:
                    n_notes += 1
                    assert note_name_to_number(m.group(1)) % 12 in scale, f"{kw}: {tok!r} is outside E-flat major"
        assert n_notes > 64 * 150


def test_min_new_tokens(golden):
    from mgea.decoder import RowSampling
    from oracle.decoder_ref import DecoderRef
    g = golden("decoder_S")
    eng, sd, n_head = make(g, max_batch=8)
    ref = DecoderRef(sd, n_head)
    rng = np.random.default_rng(61)
    prompts = rand_prompts(rng, 4, eng.vocab, 4, 12)
    n = 40
    free = eng.generate(prompts, n, 1.0, 1).cpu().tolist()
    eos = [row[3] for row in free]
    usable = [b for b in range(4) if eos[b] not in free[b][:3]]
    assert usable, "every row repeats its step-3 id earlier"
    stop = eng.generate_rows(prompts, [RowSampling(1.0, 1, eos_id=e) for e in eos], n).cpu().tolist()
    assert eng.stats()["biased_steps"] == 0
    for b in usable:
        assert stop[b][:4] == free[b][:4] and all(i == -1 for i in stop[b][4:]), f"row {b} does not stop at its EOS"
    rows = [RowSampling(1.0, 1, eos_id=e, min_new_tokens=10) for e in eos]
    got = eng.generate_rows(prompts, rows, n).cpu().tolist()
    assert eng.stats()["biased_steps"] > 0
    want, gaps = ref_biased_greedy(ref, prompts, n, None, eos, [10] * 4)
    assert exempted_rows(got, want, gaps, "min_new_tokens") == 0
    for b in usable:
        assert got[b][:3] == free[b][:3] and got[b][3] != eos[b]
        produced = [i for i in got[b] if i >= 0]
        assert len(produced) >= 10 and eos[b] not in produced[:10]
        if eos[b] in produced:
            assert produced.index(eos[b]) == len(produced) - 1
    # the same through generate_biased(): one eos for all rows
    e0 = eos[usable[0]]
    a = eng.generate_biased(prompts, n, 1.0, 1, eos_id=e0, min_new_tokens=10).cpu().tolist()
    w, gp = ref_biased_greedy(ref, prompts, n, None, [e0] * 4, [10] * 4)
    assert exempted_rows(a, w, gp, "min_new_tokens through generate_biased()") == 0
    with pytest.raises(ValueError, match="min_new_tokens"):
        eng.generate_biased(prompts, n, 1.0, 1, min_new_tokens=n + 1)


def test_sampled_biased_replay_through_step(golden):
    from mgea import ops
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    eng, _, _ = make(g, max_batch=8)
    V = eng.vocab
    rng = np.random.default_rng(67)
    prompts = rand_prompts(rng, 4, V, 4, 9)
    B, Tp, n_steps, seed, temp = 4, max(len(q) for q in prompts), 40, 4321, 0.9
    bias = make_bias(rng, "mixed", (B, V))
    idx = torch.zeros(B, Tp, dtype=torch.long)
    for b, q in enumerate(prompts):
        idx[b, :len(q)] = torch.tensor(q)
    lens = torch.tensor([len(q) for q in prompts])

    def replay(ids, pen):
        eng.reset_and_prefill(idx, lens, want_logits=False, max_len=Tp + n_steps)
        seen = [set(q) for q in prompts]
        fed = torch.tensor([q[-1] for q in prompts], dtype=torch.int32)
        rows = [RowSampling(temp, 50, None, pen, seed=seed) for _ in range(B)]
        for s in range(n_steps):
            _, lg = eng.step(fed, eng.sampler(1.0, 1), want_logits=True)
            got = ops.sample_rows(lg, rows, step=s, presence=[sorted(x) for x in seen], logit_bias=bias).cpu().tolist()
            assert got == ids[:, s].tolist(), f"penalty {pen}: step {s}: replay {got} vs generate {ids[:, s].tolist()}"
            for b in range(B):
                seen[b].add(int(ids[b, s]))
            fed = ids[:, s].to(torch.int32)

    plain = eng.generate(prompts, n_steps, temp, 50, seed=seed).cpu()
    out = eng.generate_biased(prompts, n_steps, temp, 50, seed=seed, logit_bias=bias).cpu()
    assert not torch.equal(out, plain)
    replay(out, None)
    both = eng.generate_biased(prompts, n_steps, temp, 50, seed=seed, logit_bias=bias, repetition_penalty=1.3).cpu()
    assert not torch.equal(both, out)
    assert eng.stats()["biased_steps"] == n_steps and eng.stats()["penalized_steps"] == n_steps
    replay(both, 1.3)


def test_launch_forms_agree(golden):
    from mgea import _lib
    g = golden("decoder_S")
    rng = np.random.default_rng(71)
    V = int(g["cfg"][1])
    prompts4 = rand_prompts(rng, 4, V, 5, 9)
    prompts1 = prompts4[:1]
    bias = make_bias(rng, "mixed", V)
    n = 70

    def run(switches, prompts, **kw):
        old = {k: _lib.tune_set(k, v) for k, v in switches.items()}   # (the engine switches are latched at create)
        try:
            eng, _, _ = make(g, max_batch=8)
            out = eng.generate_biased(prompts, n, 1.0, logit_bias=bias, min_new_tokens=20, eos_id=5, **kw).cpu()
            assert eng.stats()["biased_steps"] > 0
            eng.close()
            return out
        finally:
            for k, v in old.items():
                _lib.tune_set(k, v)

    for prompts in (prompts4, prompts1):
        base = run({}, prompts, top_k=1, repetition_penalty=1.2)
        assert torch.equal(base, run({"decoder_unfused": 1}, prompts, top_k=1, repetition_penalty=1.2))
        assert torch.equal(base, run({"decoder_nograph": 1}, prompts, top_k=1, repetition_penalty=1.2))
        if len(prompts) == 1:
            assert torch.equal(base, run({"decoder_nogemv": 1}, prompts, top_k=1, repetition_penalty=1.2))
    a = run({"decoder_graph_steps": 1}, prompts4, top_k=50, seed=5)
    b = run({"decoder_graph_steps": 8}, prompts4, top_k=50, seed=5)
    assert torch.equal(a, b)

    eng, _, _ = make(g, max_batch=8)
    want = eng.generate_biased(prompts4[:3], 40, 1.0, 1, logit_bias=bias).cpu()
    eng.profile(7)
    got = eng.generate_biased(prompts4[:3], 40, 1.0, 1, logit_bias=bias).cpu()
    eng.profile(0)
    eng.profile_read()
    assert torch.equal(want, got)


def test_graph_reuse_across_bias_values(golden):
    g = golden("decoder_S")
    rng = np.random.default_rng(73)
    V = int(g["cfg"][1])
    prompts = rand_prompts(rng, 4, V, 5, 9)
    eng, _, _ = make(g, max_batch=8)
    eng.generate_biased(prompts, 70, 1.0, top_k=50, seed=5, logit_bias=make_bias(rng, "finite", V))
    inst = eng.stats()["graph_instantiates"]
    other = make_bias(rng, "mixed", (4, V))
    again = eng.generate_biased(prompts, 70, 0.8, top_k=50, top_p=0.9, seed=77, logit_bias=other, min_new_tokens=30, eos_id=9,
                         repetition_penalty=1.4).cpu()
    assert eng.stats()["graph_instantiates"] == inst, "new bias values / min_new_tokens must replay the cached graph"
    only_min = eng.generate_biased(prompts, 70, 0.8, top_k=50, seed=78, min_new_tokens=30, eos_id=9).cpu()
    assert eng.stats()["graph_instantiates"] == inst
    fresh, _, _ = make(g, max_batch=8)
    assert torch.equal(only_min, fresh.generate_biased(prompts, 70, 0.8, top_k=50, seed=78, min_new_tokens=30, eos_id=9).cpu())
    assert torch.equal(again, fresh.generate_biased(prompts, 70, 0.8, top_k=50, top_p=0.9, seed=77, logit_bias=other, min_new_tokens=30,
                                             eos_id=9, repetition_penalty=1.4).cpu())
    # every form of one batch size, single-step and 8-step graphs, fits the cache: nothing is captured twice
    for _ in range(2):
        eng.generate(prompts, 70, 1.0, 1)
        eng.generate(prompts, 70, 1.0, 50, seed=1)
        eng.generate(prompts, 70, 1.0, 1, repetition_penalty=1.2)
        eng.generate(prompts, 70, 1.0, 50, seed=1, repetition_penalty=1.2)
        eng.generate_biased(prompts, 70, 1.0, 1, logit_bias=other)
        eng.generate_biased(prompts, 70, 1.0, 50, seed=1, logit_bias=other)
        once = eng.stats()["graph_instantiates"] if _ == 0 else once
    assert eng.stats()["graph_instantiates"] == once


def test_unbiased_paths_untouched_and_mixed_batches(golden):
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    rng = np.random.default_rng(79)
    V = int(g["cfg"][1])
    prompts = rand_prompts(rng, 4, V, 5, 9)
    bias = make_bias(rng, "mixed", V)
    eng, _, _ = make(g, max_batch=8)
    fresh, _, _ = make(g, max_batch=8)
    want = fresh.generate(prompts, 50, 1.0, 1).cpu()
    nodes = fresh.stats()["graph_nodes"]
    want_s = fresh.generate(prompts, 50, 1.0, 50, seed=2).cpu()
    nodes_s = fresh.stats()["graph_nodes"]
    want_p = fresh.generate(prompts, 50, 1.0, 1, repetition_penalty=1.3).cpu()
    nodes_p = fresh.stats()["graph_nodes"]
    want_ps = fresh.generate(prompts, 50, 1.0, 50, seed=2, repetition_penalty=1.3).cpu()
    eng.generate_biased(prompts, 50, 1.0, 1, logit_bias=bias)
    eng.generate_biased(prompts, 50, 1.0, 50, seed=2, logit_bias=bias, min_new_tokens=7, eos_id=3, repetition_penalty=1.3)
    assert eng.stats()["biased_steps"] > 0
    got = eng.generate(prompts, 50, 1.0, 1).cpu()
    assert torch.equal(got, want) and eng.stats()["graph_nodes"] == nodes and eng.stats()["biased_steps"] == 0
    with pytest.raises(RuntimeError):     # an unprocessed generate keeps no presence bitmaps
        eng.presence()
    got = eng.generate(prompts, 50, 1.0, 50, seed=2).cpu()
    assert torch.equal(got, want_s) and eng.stats()["graph_nodes"] == nodes_s and eng.stats()["biased_steps"] == 0
    got = eng.generate(prompts, 50, 1.0, 1, repetition_penalty=1.3).cpu()
    st = eng.stats()
    assert torch.equal(got, want_p) and st["graph_nodes"] == nodes_p and st["biased_steps"] == 0 and st["penalized_steps"] == 50
    assert torch.equal(eng.generate(prompts, 50, 1.0, 50, seed=2, repetition_penalty=1.3).cpu(), want_ps)

    # a mixed batch: the rows without a bias are the rows of an all-unbiased batch of that size, greedy and sampled
    for k, pen in ((1, None), (50, None), (50, 1.3)):
        base = [RowSampling(0.9, k, None, pen, seed=11 + b, stream=b) for b in range(4)]
        plain = eng.generate_rows(prompts, base, 50).cpu()
        mixed = [RowSampling(0.9, k, None, pen, seed=11 + b, stream=b, logit_bias=bias if b in (0, 3) else None) for b in range(4)]
        out = eng.generate_rows(prompts, mixed, 50).cpu()
        assert eng.stats()["biased_steps"] == 50
        assert torch.equal(out[1], plain[1]) and torch.equal(out[2], plain[2]), f"top_k={k} penalty={pen}"
        assert not torch.equal(out[0], plain[0])
        assert np.isfinite(bias[out[0].numpy()]).all() and np.isfinite(bias[out[3].numpy()]).all()
        # ... and a row's ids go with its (prompt, record), not with its index
        perm = [3, 2, 1, 0]
        swapped = eng.generate_rows([prompts[i] for i in perm], [mixed[i] for i in perm], 50).cpu()
        assert torch.equal(swapped, out[perm]), f"top_k={k} penalty={pen}"


def test_f16_engine_biased_top_p():
    from mgea.decoder import DecoderEngine
    V, L, C, NL = 8324, 2112, 768, 12
    sd = synth.decoder_state_dict(41, V, L, C, NL)
    eng = DecoderEngine(sd, n_head=12, max_batch=8, max_ctx=L, dtype="f16")
    rng = np.random.default_rng(83)
    prompts = rand_prompts(rng, 8, V, 16, 48)
    ban = make_bias(rng, "ban70", V)
    n = 2048
    a = eng.generate_biased(prompts, n, 1.0, top_k=0, top_p=0.9, seed=3, repetition_penalty=1.1, logit_bias=ban).cpu()
    st = eng.stats()
    assert st["graph_replays"] == n and st["biased_steps"] == n and st["penalized_steps"] == n and st["graph_nodes"] > 0
    b = eng.generate_biased(prompts, n, 1.0, top_k=0, top_p=0.9, seed=3, repetition_penalty=1.1, logit_bias=ban).cpu()
    assert torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < V
    assert np.isfinite(ban[a.numpy()]).all(), "a banned id was drawn"


# ---------------------------------------------------------------------------------------------------------- end to end
def test_constrained_endpoint_end_to_end(golden):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_app, create_batched_app, create_constrained_app
    from emotion_analysis import EATS, inference
    from generate_music import constraints
    from generate_music.midi import note_name_to_number, note_re
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer

    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=8, max_ctx=256)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))

    def check(app, constrain):
        client = TestClient(app)
        seen = []
        app.state.on_tokens = seen.append
        kw = {"data": {"prompt": "i love life"}} if app.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
        random.seed(3)
        r = client.post("/generate", **kw)
        assert r.status_code == 200 and r.headers["content-type"].startswith("audio/midi") and r.content[:4] == b"MThd"
        assert r.headers["X-Constraint"] == constrain
        assert model.engine.stats()["biased_steps"] > 0
        key = EATS.get_music_params(r.headers["X-Emotion"])["key"]
        scale = constraints.scale_pitch_classes(key)
        tokens = seen[-1]
        n_prompt = int(r.headers["X-Prompt-Tokens"])
        new = tokens[n_prompt:]
        assert len(new) >= 12                      # min_new_tokens
        n_notes = 0
        for tok in new:
            m = note_re.match(tok)
            assert m or tok.startswith("[INSTRUMENT]") or tok == "[END_SEQUENCE]", f"control token {tok!r} after the prompt"
            if m:
                n_notes += 1
                if constrain == "scale":
                    assert note_name_to_number(m.group(1)) % 12 in scale, f"{tok!r} is outside {key}"
        assert n_notes > 0

    check(create_constrained_app(model, seq_len=64, temperature=1.0, top_k=0, top_p=0.92, repetition_penalty=1.1, constrain="scale",
                     min_new_tokens=12), "scale")
    check(create_constrained_app(model, seq_len=64, temperature=1.0, top_k=50, constrain="notes", min_new_tokens=12), "notes")
    app = create_batched_app(model, seq_len=64, temperature=1.0, top_k=50, constrain="scale", min_new_tokens=12)
    try:
        check(app, "scale")
    finally:
        app.state.batcher.close()
    plain = create_app(model, seq_len=64, temperature=1.0, top_k=50)
    client = TestClient(plain)
    kw = {"data": {"prompt": "i love life"}} if plain.state.prompt_in == "form" else {"params": {"prompt": "i love life"}}
    r = client.post("/generate", **kw)
    assert r.status_code == 200 and "X-Constraint" not in r.headers and model.engine.stats()["biased_steps"] == 0
