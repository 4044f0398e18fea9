"""Every per-row record table of a generation under mirroring, in one call on the MI355X.  A guidance shadow row and the members of a
blend group run on their source row's inputs (csrc/gen_plan.h: mirror_sources; csrc/decoder_generate.hip: mirror_shadow_rows): the
sampler record, the grammar start state, the truncation record, the class-penalty record, the bias vector, the forced ids and the
presence bitmap.  A table that the mirror leaves out is a silent wrong answer, so the mirrored rows are handed DECOY records here --
each one valid and switched on, each one different from the source's -- and the call must behave, exactly, as the same call with
the source's records on those rows.  Through the raw ABI (mgea_decoder_generate_rows_class_penalized, the end of the chain): the
Python wrappers fill a mirrored row with its source's records themselves.

The batch of 6: a pair (row 0, shadow row 4), a group (leader 1, members 2 and 5), a plain row 3.  Every assertion is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu
B, TP, N_STEPS = 6, 3, 8
SOURCE = {2: 1, 4: 0, 5: 1}             # mirrored row -> the row whose inputs it takes
FORCED_STEPS = (2, 5)
GUIDE = [(4, 1.5)] + [(-1, 0.0)] * 5
BLEND = [(-1, 0.0), (1, 0.6), (1, 0.3), (-1, 0.0), (-1, 0.0), (1, 0.1)]


def parity_at(start, step):
    """the grammar alternates between the even (state 0) and the odd ids (state 1): what a row that started in `start` may take at `step`"""
    return (start + step) % 2


def records(vocab, decoy_rows):
    """per row: (sampler, truncation, class penalty, start state, bias vector, forced ids); rows in decoy_rows get the decoy of the
    record their source (or, for a row that has none, they themselves) would have"""
    rng = np.random.default_rng(97)
    bias = (rng.standard_normal((2, B, vocab)) * 2).astype(np.float32)      # [0] the sources' vectors, [1] the decoys'
    ids = rng.integers(0, vocab // 2 - 1, (2, B, len(FORCED_STEPS)))
    out = []
    for b in range(B):
        d = 1 if b in decoy_rows else 0
        src = SOURCE.get(b, b)          # a record is a function of the row whose record it is, so that "the source's record" is one thing
        start = (src + d) % 2
        forced = [-1] * N_STEPS
        for j, s in enumerate(FORCED_STEPS):
            forced[s] = 2 * int(ids[d, src, j]) + parity_at(start, s)
        out.append(dict(sampler=dict(temperature=(1.0, 0.7)[d], top_k=20, repetition_penalty=1.2, seed=(11, 23)[d] + src, stream=src + 16 * d),
                        trunc=((0.05, 0.0, 0.0, 0.0), (0.3, 0.9, 0.0, 0.0))[d], cpen=((0.5, 2.0, 4), (-0.25, 1.0, 2))[d], start=start,
                        bias=bias[d, src], forced=forced))
    return out


def run(eng, recs):
    """the call on `recs`; returns (ids, logprobs, choice logprobs, grammar states, presence words, error flags)"""
    from mgea import _lib, ops
    from mgea.decoder import RowSampling, pack_rows
    prompts = synth.integers(5, "row_tables", (B, TP), 0, eng.vocab).astype(np.int32)
    ids = torch.from_numpy(prompts).cuda().contiguous()
    bias = torch.from_numpy(np.stack([r["bias"] for r in recs])).cuda().contiguous()
    forced = torch.tensor([r["forced"] for r in recs], dtype=torch.int32, device="cuda").contiguous()
    out = torch.empty(B, N_STEPS, dtype=torch.int32, device="cuda")
    lp = torch.zeros(B, N_STEPS, dtype=torch.float32, device="cuda")
    ch = torch.zeros(B, N_STEPS, dtype=torch.float32, device="cuda")
    states = torch.empty(B, dtype=torch.int32, device="cuda")
    words = torch.empty(B, ops.presence_words(eng.vocab), dtype=torch.int32, device="cuda")
    srecs = pack_rows([RowSampling(**r["sampler"]) for r in recs], eng.vocab, N_STEPS)
    lrecs = (_lib.RowLogits * B)(*[_lib.RowLogits(bias_dev=bias[b].data_ptr(), min_new_tokens=0, reserved=0) for b in range(B)])
    starts = (C.c_int32 * B)(*[r["start"] for r in recs])
    garr = (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in GUIDE])
    barr = (_lib.RowBlend * B)(*[_lib.RowBlend(leader=l, weight=w) for l, w in BLEND])
    tarr = (_lib.RowTruncation * B)(*[_lib.RowTruncation(*r["trunc"]) for r in recs])
    carr = (_lib.RowClassPenalty * B)(*[_lib.RowClassPenalty(frequency=r["cpen"][0], presence=r["cpen"][1], window=r["cpen"][2], reserved=0)
                                        for r in recs])
    flags = C.c_int32(0)
    torch.cuda.synchronize()
    with eng._on_stream():
        rc = eng.lib.mgea_decoder_generate_rows_class_penalized(eng.h, _lib.ptr(ids), None, B, TP, N_STEPS, srecs, lrecs, starts, garr, None, 1,
                                                                _lib.ptr(forced), _lib.ptr(out), _lib.ptr(lp), _lib.ptr(ch), tarr, barr, carr,
                                                                eng._sp())
        assert rc == 0, _lib.last_error()
        _lib.check(eng.lib.mgea_decoder_grammar_states(eng.h, _lib.ptr(states), eng._sp()))
        _lib.check(eng.lib.mgea_decoder_presence(eng.h, _lib.ptr(words), eng._sp()))
        _lib.check(eng.lib.mgea_decoder_error_flags(eng.h, C.byref(flags), eng._sp()))
    torch.cuda.synchronize()
    return out.cpu(), lp.cpu(), ch.cpu(), states.cpu(), words.cpu(), flags.value


@pytest.mark.parametrize("mode", ["graphs", "nograph"])
def test_mirrored_rows_take_every_table_of_their_source(tune, mode):
    from mgea.decoder import DecoderEngine
    from test_gpu_guidance import grammar_of
    tune("decoder_nograph", 1 if mode == "nograph" else 0)   # latched when an engine is created
    sd = synth.decoder_state_dict(11, 311, 64, 256, 2)
    eng = DecoderEngine(sd, n_head=4, max_batch=8, max_ctx=64, device="cuda:0")
    eng.set_grammar(grammar_of(eng.vocab))
    eng.set_penalty_classes(np.arange(eng.vocab) % 12)
    source, decoyed = records(eng.vocab, ()), records(eng.vocab, set(SOURCE))
    for u, b in SOURCE.items():   # the decoys differ from the source's records in every table, and are on
        s, d = source[u], decoyed[u]
        assert s["sampler"] == source[b]["sampler"] and s["forced"] == source[b]["forced"]
        assert all(d["sampler"][k] != s["sampler"][k] for k in ("seed", "stream", "temperature"))
        assert d["trunc"] != s["trunc"] and d["trunc"][0] > 0 and d["cpen"] != s["cpen"] and d["cpen"][1] != 0
        assert d["start"] != s["start"] and not np.array_equal(d["bias"], s["bias"])
        assert all(d["forced"][t] >= 0 and d["forced"][t] != s["forced"][t] for t in FORCED_STEPS)
    got = run(eng, decoyed)
    assert (eng.stats()["graph_instantiates"] == 0) == (mode == "nograph")
    want = run(eng, source)
    assert eng.guidance_info() == dict(pairs=1, guided_steps=N_STEPS) and eng.blend_info() == dict(groups=1, rows=3, blended_steps=N_STEPS)
    assert eng.class_penalty_info() == dict(n_class=12, rows=B, class_penalized_steps=N_STEPS)
    assert eng.truncation_info()["rows"] == B and eng.grammar_info()["grammar_steps"] == N_STEPS
    ids = got[0]
    assert int(ids.min()) >= 0 and got[5] == 0 and want[5] == 0, "a forced id was banned by the grammar state its row ran in"
    for b in range(B):            # the forced steps took their ids: the sources' ones
        for t in FORCED_STEPS:
            assert int(ids[b, t]) == source[b]["forced"][t], f"{mode}: row {b} step {t} did not take its source's forced id"
    for u, b in SOURCE.items():   # 1. a mirrored row returns its source row's ids
        assert torch.equal(ids[u], ids[b]), f"{mode}: row {u} left its source row {b}: {ids[u].tolist()} vs {ids[b].tolist()}"
    for name, g, w in zip(("ids", "log-probabilities", "choice log-probabilities", "grammar states", "presence bitmaps"), got, want):
        assert g.numpy().tobytes() == w.numpy().tobytes(), f"{mode}: {name} differ from the call with the sources' records on rows 2, 4 and 5"   # 2.
    # 3. the decoy is one: on row 3, which nothing mirrors, it changes the ids
    plain = run(eng, records(eng.vocab, {3}))
    free = [t for t in range(N_STEPS) if t not in FORCED_STEPS]
    assert not torch.equal(plain[0][3, free], want[0][3, free]), f"{mode}: row 3 draws the same ids from the decoy record"
    for b in (0, 1, 2, 4, 5):     # (and row 3's record reaches no other row)
        assert torch.equal(plain[0][b], want[0][b])
    eng.close()
