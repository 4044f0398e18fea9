"""The four launch sequences of the decode step's tail (StepForm in csrc/gen_plan.h: greedy, sampled, penalized, biased), on the fused
5-launch path (decoder_tiny8h, d_model 256) and the unfused one (decoder_tiny, d_model 128): captured graphs against eager launches,
the graph cache keyed on the form alone, and the sampler's two ways of receiving its scalars (by value, device records).
12 steps with the default 8 steps per graph: one 8-step graph launch, then the single-step graph four times."""
import ctypes as C

import numpy as np
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu
N_STEPS = 12
EOS = 2
FORMS = ("greedy", "sampled", "penalized", "biased")


def make(g, **kw):
    from mgea.decoder import DecoderEngine
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return DecoderEngine(sd, n_head=n_head, max_batch=4, max_ctx=seq_len, **kw)


def case(golden, tag):
    """B = 2 ragged prompts (3-5 tokens) and a dense finite bias, N(0, 2) per id"""
    g = golden("decoder_" + tag)
    prompts = [g["prompt0"].tolist(), g["prompt1"].tolist()]
    assert len({len(p) for p in prompts}) == 2 and all(3 <= len(p) <= 5 for p in prompts)
    bias = (np.random.default_rng(5).standard_normal(int(g["cfg"][1])) * 2).astype(np.float32)
    return g, prompts, bias


def run_form(eng, form, prompts, bias, top_k=20):
    if form == "greedy":
        return eng.generate(prompts, N_STEPS, 1.0, top_k=1).cpu()
    if form == "sampled":
        return eng.generate(prompts, N_STEPS, 1.0, top_k=top_k, seed=7).cpu()
    if form == "penalized":
        return eng.generate(prompts, N_STEPS, 1.0, top_k=top_k, seed=7, repetition_penalty=1.2).cpu()
    return eng.generate_biased(prompts, N_STEPS, 1.0, top_k=top_k, seed=7, eos_id=EOS, repetition_penalty=1.2, logit_bias=bias,
                               min_new_tokens=3).cpu()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_graphs_equal_eager_launches_in_every_form(golden, tune, tag):
    from mgea.decoder import RowSampling
    g, prompts, bias = case(golden, tag)
    eng = make(g)
    got = {f: run_form(eng, f, prompts, bias) for f in FORMS}
    assert eng.stats()["graph_instantiates"] > 0
    rows = [RowSampling(1.0, 20, None, 1.2, EOS, 0, 7, None, bias, 3) for _ in prompts]
    assert torch.equal(eng.generate_rows(prompts, rows, N_STEPS).cpu(), got["biased"])
    assert eng.stats()["biased_steps"] > 0
    eng.close()
    tune("decoder_nograph", 1)   # latched when an engine is created
    eager = make(g)
    for f in FORMS:
        want = run_form(eager, f, prompts, bias)
        assert want.shape == (2, N_STEPS) and int(want.max()) < eager.vocab
        assert torch.equal(got[f], want), f"{tag}: the {f} form's graphs and its eager launches give different ids"
    assert eager.stats()["graph_instantiates"] == 0
    eager.close()


@pytest.mark.parametrize("tag", ["tiny8h", "tiny"])
def test_one_graph_set_per_form(golden, tag):
    from mgea import _lib
    g, prompts, bias = case(golden, tag)
    per = 2 if _lib.tune_get("decoder_graph_steps") > 1 else 1   # a form's single-step graph and (12 steps >= 8) its 8-step graph
    eng = make(g)
    run_form(eng, "penalized", prompts, bias)
    inst = eng.stats()["graph_instantiates"]
    assert inst == per
    greedy_pen = run_form(eng, "penalized", prompts, bias, top_k=1)   # the same launch sequence: every scalar is in the records
    assert eng.stats()["graph_instantiates"] == inst, "a penalized top_k = 1 generation captured a twin of the penalized graphs"
    fresh = make(g)
    assert torch.equal(greedy_pen, run_form(fresh, "penalized", prompts, bias, top_k=1))
    fresh.close()
    for f in ("greedy", "sampled", "biased"):
        run_form(eng, f, prompts, bias)
    assert eng.stats()["graphs_cached"] == 4 * per and eng.stats()["graph_instantiates"] == 4 * per
    for f in FORMS:
        run_form(eng, f, prompts, bias)
    run_form(eng, "biased", prompts, bias, top_k=1)
    assert eng.stats()["graph_instantiates"] == 4 * per
    eng.close()


def test_records_equal_by_value_scalars():
    """[3, 300] logits: the same settings on every row as device records (stream = b) and by value -- same ids, same pre-draw
    probabilities, bitwise; through mgea_op_sample, _penalized, _rows and _rows_biased"""
    from mgea import _lib, ops
    from mgea.decoder import RowSampling
    rng = np.random.default_rng(11)
    B, V, step = 3, 300, 5
    logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32)).cuda()
    mask = torch.from_numpy(rng.random((B, V)) < 0.1)
    for temp, k, tp in ((1.0, 20, None), (0.8, None, 0.9), (1.3, 20, 0.9)):
        for pen in (None, 1.2):
            ids, p = ops.sample(logits, temp, k, tp, seed=42, step=step, want_probs=True, repetition_penalty=pen, presence=mask)
            rows = [RowSampling(temp, k, tp, pen, eos_id=EOS, seed=42, stream=b) for b in range(B)]
            r_ids, r_p = ops.sample_rows(logits, rows, step=step, want_probs=True, presence=mask)
            assert torch.equal(ids, r_ids) and torch.equal(p, r_p)
            # the BIAS kernel with nothing left for it to do: no bias vector, and a min_new_tokens that the step has passed
            b_ids, b_p = ops.sample_rows(logits, rows, step=step, want_probs=True, presence=mask, min_new_tokens=step)
            assert torch.equal(ids, b_ids) and torch.equal(p, b_p)
    # a penalty of exactly 1 needs no bitmap: NULL is accepted and the call is mgea_op_sample
    lib = _lib.load()
    s = _lib.SamplerConfig(temperature=1.0, top_k=20, top_p=0.0, eos_id=-1, seed=42)
    want_ids, want_p = ops.sample(logits, 1.0, 20, None, seed=42, step=step, want_probs=True)
    ids = torch.empty(B, dtype=torch.int32, device="cuda")
    p = torch.empty(B, V, dtype=torch.float32, device="cuda")
    rc = lib.mgea_op_sample_penalized(_lib.ptr(logits), B, V, C.byref(s), 1.0, None, step, _lib.ptr(ids), _lib.ptr(p), _lib.stream_ptr())
    assert rc == 0, _lib.load().mgea_last_error()
    assert torch.equal(ids, want_ids) and torch.equal(p, want_p)
