"""The nine mgea_decoder_generate_rows* entry points are one request with some fields left out (GenRequest, csrc/gen_plan.h): each is
called directly through ctypes, then again through mgea_decoder_generate_rows_class_penalized -- the superset at the end of the chain,
the one call DecoderEngine._run_rows makes -- with NULL (or n_seg_max = 1) for what it lacks.  Both calls must give the same ids, log-probabilities and report, bit for
bit, and the second one must replay the first one's graphs: the same step kind, so the same graph key.
On the fused path (decoder_tiny8h, d_model 256) and the unfused one (decoder_tiny, d_model 128); 12 steps = one 8-step graph launch
plus four single-step replays, as in test_gpu_step_forms.py.
In the library every one of these entry points builds its request in one file-local function (csrc/decoder_generate.hip:
generate_rows), so what this test holds is the argument order and the NULL defaults of each exported signature."""
import ctypes as C

import numpy as np
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu
N_STEPS = 12
EOS = 2
ENTRY_POINTS = ("rows", "rows_biased", "rows_scored", "rows_grammar", "rows_guided", "rows_scheduled", "rows_truncated", "rows_blended",
                "rows_class_penalized")


def make(g):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=4, max_ctx=seq_len)


def parity_grammar(vocab):
    """even ids and odd ids in turn: state 0 admits the even ids and goes to 1, state 1 the odd ids and goes back"""
    from mgea.decoder import TokenGrammar
    return TokenGrammar(np.arange(vocab) % 2, np.array([[1, -1], [-1, 0]]))


def request(eng, g, name):
    """Every argument of mgea_decoder_generate_rows_class_penalized for the case of entry point `name`, None / 1 where that one has no such
    argument, as a dict; plus the tensors the records point into."""
    from mgea import _lib
    from mgea.decoder import (ClassPenalty, RowSampling, RowSchedule, Truncation, pack_class_penalty, pack_row_logits, pack_rows,
                              pack_truncation)
    p0, p1 = g["prompt0"].tolist(), g["prompt1"].tolist()
    assert len(p0) != len(p1) and all(3 <= len(p) <= 5 for p in (p0, p1))
    paired = name in ("rows_guided", "rows_scheduled", "rows_blended")
    if paired:   # B = 4: two 8-token prompts, and behind them their shadow rows (or members), the prompts without their first two tokens
        c0, c1 = (p0 + p1 + p0)[:8], (p1 + p0 + p1)[:8]
        prompts = [c0, c1, c0[2:], c1[2:]]
    else:        # B = 2: ragged prompts of 3-5 tokens
        prompts = [p0, p1]
    B, Tp = len(prompts), max(len(p) for p in prompts)
    ids = torch.zeros(B, Tp, dtype=torch.int32)
    for b, p in enumerate(prompts):
        ids[b, :len(p)] = torch.tensor(p, dtype=torch.int32)
    a = dict(B=B, Tp=Tp, lens=torch.tensor([len(p) for p in prompts], dtype=torch.int32).cuda(), lrecs=None, starts=None, guide=None,
             sched=None, n_seg_max=1, forced=None, scored=False, trunc=None, blend=None, cpen=None)
    biased = name != "rows"
    bias = (np.random.default_rng(5).standard_normal(eng.vocab) * 2).astype(np.float32) if biased else None
    eos = -1 if paired else EOS   # (a row that drew its EOS id before step 5 would not switch)
    rows = [RowSampling(1.0, 20, None, 1.2 if biased else 1.0, eos, 0, 7 + b, None, bias, 3 if biased else 0) for b in range(B)]
    if paired:   # a shadow row, or a member, is a plain row (its conditional row's, or its leader's, record replaces its own)
        rows[2:] = [RowSampling(), RowSampling()]
    if name == "rows_blended":   # groups {0, 2} and {1, 3}
        a["blend"] = (_lib.RowBlend * B)(_lib.RowBlend(0, 0.6), _lib.RowBlend(1, 1.5), _lib.RowBlend(0, 0.4), _lib.RowBlend(1, -0.5))
    elif paired:
        a["guide"] = (_lib.RowGuidance * B)(_lib.RowGuidance(2, 1.5), _lib.RowGuidance(3, 0.5), _lib.RowGuidance(-1, 0.0),
                                            _lib.RowGuidance(-1, 0.0))
    if name == "rows_truncated":   # row 0 only; row 1 gets a record that is all off
        rows[0].truncation = Truncation(min_p=0.05, typical_p=0.9)
        a["trunc"] = pack_truncation(rows)
    if name == "rows_class_penalized":   # row 0 on, row 1 an off record
        eng.set_penalty_classes(np.arange(eng.vocab) % 4)
        rows[0].class_penalty, rows[1].class_penalty = ClassPenalty(0.5, 1.0, 4), ClassPenalty()
        a["cpen"] = pack_class_penalty(rows, N_STEPS, 4)
    a["recs"] = pack_rows(rows, eng.vocab, N_STEPS)
    a["lrecs"], keep = pack_row_logits(rows, eng.vocab, eng.device)
    if name in ("rows_scored", "rows_grammar", "rows_scheduled", "rows_truncated"):
        a["scored"] = True
        forced = torch.full((B, N_STEPS), -1, dtype=torch.int32)
        forced[0, 1], forced[1, 9] = 11, 4
        a["forced"] = forced.cuda()
    if name in ("rows_grammar", "rows_scheduled"):
        eng.set_grammar(parity_grammar(eng.vocab))
        a["starts"] = (C.c_int32 * B)(*([0, 1, -1, -1][:B]))
    if name == "rows_scheduled":   # row 0 switches to its second variant at step 5, row 1 never does; the shadows have one variant
        second = ids.clone()
        second[0, :3] = torch.tensor(list(reversed(prompts[0][:3])), dtype=torch.int32)
        ids = torch.stack([ids, second], dim=0)
        a["sched"] = (_lib.RowSchedule * B)(RowSchedule([5]).record(), *[RowSchedule().record() for _ in range(B - 1)])
        a["n_seg_max"] = 2
    a["ids"] = ids.cuda().contiguous()
    return a, keep


def call(eng, a, name):
    """One generation through entry point `name` (the direct call) or "superset" (mgea_decoder_generate_rows_class_penalized): the ids, the
    log-probabilities where scored, and everything the engine reports about the call."""
    from mgea._lib import check, ptr
    lib, h, sp = eng.lib, eng.h, eng._sp()
    B, scored = a["B"], a["scored"]
    out = torch.full((B, N_STEPS), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((B, N_STEPS), 7.0, device="cuda") if scored else None
    ch = torch.full((B, N_STEPS), 7.0, device="cuda") if scored else None
    head = (h, ptr(a["ids"]), ptr(a["lens"]), B, a["Tp"], N_STEPS, a["recs"])
    tail = (ptr(a["forced"]), ptr(out), ptr(lp), ptr(ch), sp)
    with eng._on_stream():
        if name == "rows":
            check(lib.mgea_decoder_generate_rows(*head, ptr(out), sp))
        elif name == "rows_biased":
            check(lib.mgea_decoder_generate_rows_biased(*head, a["lrecs"], ptr(out), sp))
        elif name == "rows_scored":
            check(lib.mgea_decoder_generate_rows_scored(*head, a["lrecs"], *tail))
        elif name == "rows_grammar":
            check(lib.mgea_decoder_generate_rows_grammar(*head, a["lrecs"], a["starts"], *tail))
        elif name == "rows_guided":
            check(lib.mgea_decoder_generate_rows_guided(*head, a["lrecs"], a["starts"], a["guide"], *tail))
        else:
            mid = (a["lrecs"], a["starts"], a["guide"], a["sched"], a["n_seg_max"], *tail[:-1])
            if name == "rows_scheduled":
                check(lib.mgea_decoder_generate_rows_scheduled(*head, *mid, sp))
            elif name == "rows_truncated":
                check(lib.mgea_decoder_generate_rows_truncated(*head, *mid, a["trunc"], sp))
            elif name == "rows_blended":
                check(lib.mgea_decoder_generate_rows_blended(*head, *mid, a["trunc"], a["blend"], sp))
            else:
                assert name in ("rows_class_penalized", "superset")
                check(lib.mgea_decoder_generate_rows_class_penalized(*head, *mid, a["trunc"], a["blend"], a["cpen"], sp))
    eng._cur_batch = B
    report = dict(stats=eng.stats(), grammar=eng.grammar_info(), guidance=eng.guidance_info(), schedule=eng.schedule_info(),
                  truncation=eng.truncation_info(), blend=eng.blend_info(), class_penalty=eng.class_penalty_info())
    assert eng.id_errors(raise_error=False) == 0
    return out.cpu(), None if lp is None else lp.cpu(), None if ch is None else ch.cpu(), report


@pytest.mark.parametrize("name", ENTRY_POINTS)
@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_entry_point_equals_the_superset_call(golden, tag, name):
    g = golden("decoder_" + tag)
    eng = make(g)
    a, keep = request(eng, g, name)
    torch.cuda.synchronize()   # the uploads ran on the caller's stream
    ids, lp, ch, rep = call(eng, a, name)
    assert ids.shape == (a["B"], N_STEPS) and int(ids.max()) < eng.vocab and int(ids.min()) >= -1 and bool((ids[:, 0] >= 0).all())
    inst = rep["stats"]["graph_instantiates"]
    assert inst > 0 and rep["stats"]["graph_replays"] > 0
    # the case is what its name says: the report shows the features the entry point exists for
    assert (rep["stats"]["biased_steps"] > 0) == (name != "rows")
    assert (rep["stats"]["scored_steps"] > 0) == a["scored"]
    assert (rep["grammar"]["grammar_steps"] > 0) == (a["starts"] is not None)
    assert rep["guidance"]["pairs"] == (2 if a["guide"] is not None else 0)
    assert (rep["schedule"]["scheduled_steps"] > 0) == (a["sched"] is not None)
    if a["sched"] is not None:
        assert rep["schedule"]["switches"] == 1
    assert (rep["truncation"]["steps"] > 0) == (a["trunc"] is not None)
    assert rep["blend"]["groups"] == (2 if a["blend"] is not None else 0)
    assert (rep["class_penalty"]["class_penalized_steps"] > 0) == (a["cpen"] is not None)
    ids2, lp2, ch2, rep2 = call(eng, a, "superset")
    assert torch.equal(ids, ids2), f"{tag}: {name} and the superset call give different ids"
    if a["scored"]:
        assert torch.equal(lp, lp2) and torch.equal(ch, ch2), f"{tag}: {name} and the superset call give different log-probabilities"
        assert bool(torch.isfinite(lp).all()) and float(lp.min()) < 0.0
    assert rep2 == rep, f"{tag}: {name} and the superset call report different generations"
    assert rep2["stats"]["graph_instantiates"] == inst, f"{tag}: the superset call captured graphs of its own: another graph key"
    del keep
    eng.close()
