"""min-p, typical-p, epsilon and eta cutoff on the CPU: the restatement of tests/truncation_util.py against transformers' warpers stage
by stage, the band case that removes a row's most likely id, the host records' refusals, and the plan of a truncated generation
(tests/native/trunc_plan_test.cpp, a stand-alone host program over csrc/gen_plan.h)."""
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import truncation_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


# ---------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("V", [97, 8324])
@pytest.mark.parametrize("case", ["min_p", "typical_lo", "typical_hi", "epsilon", "eta"])
def test_single_stage_equals_the_transformers_warper(V, case):
    lp = pytest.importorskip("transformers.generation.logits_process")
    st = tu.CASES[case]
    rng = np.random.default_rng(100 + V + 31 * list(tu.CASES).index(case))
    x = torch.from_numpy(tu.draw_robust(rng, 8, V, st))
    warper = {"min_p": lambda: lp.MinPLogitsWarper(st["min_p"]), "typical_lo": lambda: lp.TypicalLogitsWarper(st["typical_p"]),
              "typical_hi": lambda: lp.TypicalLogitsWarper(st["typical_p"]), "epsilon": lambda: lp.EpsilonLogitsWarper(st["epsilon_cutoff"]),
              "eta": lambda: lp.EtaLogitsWarper(st["eta_cutoff"])}[case]()
    hf = warper(torch.zeros(x.shape[0], 1, dtype=torch.long), x.clone())
    _, kept = tu.truncated_probs(x, st)
    assert torch.equal(torch.isfinite(hf), kept), f"V={V} {case}: kept sets differ from transformers'"
    assert 1 <= int(kept.sum(1).min()) and int(kept.sum(1).max()) < V


def test_stage_order_and_each_stage_sees_the_renormalised_set():
    """all four against the four warpers chained in the rule's order"""
    lp = pytest.importorskip("transformers.generation.logits_process")
    st = tu.CASES["all"]
    x = torch.from_numpy(tu.draw_robust(np.random.default_rng(5), 8, 8324, st))
    ids = torch.zeros(8, 1, dtype=torch.long)
    hf = x.clone()
    for w in (lp.MinPLogitsWarper(st["min_p"]), lp.TypicalLogitsWarper(st["typical_p"]), lp.EpsilonLogitsWarper(st["epsilon_cutoff"]),
              lp.EtaLogitsWarper(st["eta_cutoff"])):
        hf = w(ids, hf)
    assert torch.equal(torch.isfinite(hf), tu.truncated_probs(x, st)[1])


def band_row(V=97):
    """a spike of mass about 0.3 over a flat tail: the spike's surprise is far from the entropy, the tail's is next to it"""
    x = np.zeros((1, V), np.float32)
    x[0, 11] = math.log(0.3 / 0.7 * (V - 1))
    return x


def test_typical_p_removes_the_argmax_of_the_band_row():
    x = band_row()
    p = torch.softmax(torch.from_numpy(x).double(), -1)
    assert abs(float(p[0, 11]) - 0.3) < 1e-6
    probs, kept = tu.truncated_probs(x, dict(typical_p=0.2))
    assert not bool(kept[0, 11]) and float(probs[0, 11]) == 0.0          # the most likely id is gone
    assert int(kept.sum()) == 96 and abs(float(probs.sum()) - 1) < 1e-12  # equal d: the whole tail is the band
    assert bool(tu.robust(torch.from_numpy(x), dict(typical_p=0.2)).all())
    # min_p on the same row keeps the spike alone; epsilon above every probability keeps the largest logit, lowest id among equals
    assert torch.nonzero(tu.truncated_probs(x, dict(min_p=0.5))[1][0]).view(-1).tolist() == [11]
    flat = np.zeros((1, 97), np.float32)
    assert torch.nonzero(tu.truncated_probs(flat, dict(epsilon_cutoff=0.5))[1][0]).view(-1).tolist() == [0]
    # (eta' <= sqrt(eta) * max(p) < max(p), since H >= -log max(p): the eta stage never needs its protection, and keeps a flat row whole)
    assert int(tu.truncated_probs(flat, dict(eta_cutoff=0.9))[1].sum()) == 97
    # a banned id has mass 0 and never enters a band
    x[0, 40] = -math.inf
    assert not bool(tu.truncated_probs(x, dict(typical_p=0.2))[1][0, 40])


# ---------------------------------------------------------------------------------------------------------- the records
def test_truncation_record_and_refusals():
    from mgea.decoder import RowSampling, Truncation, pack_truncation
    t = Truncation(min_p=0.05, typical_p=0.9)
    t.check(0)
    r = t.record()
    assert (r.min_p, r.typical_p, r.epsilon_cutoff, r.eta_cutoff) == (np.float32(0.05), np.float32(0.9), 0.0, 0.0)
    assert t.on and not Truncation().on and not Truncation(typical_p=1.0).on and Truncation(eta_cutoff=1e-3).on
    assert Truncation.of() is None and Truncation.of(min_p=0.1) == Truncation(min_p=0.1)
    for kw in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=math.nan), dict(typical_p=-1), dict(typical_p=1.0001),
               dict(typical_p=math.inf), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1e-3), dict(eta_cutoff=1.0),
               dict(eta_cutoff=math.nan)):
        with pytest.raises(ValueError, match=f"row 3: {next(iter(kw))}"):
            Truncation(**kw).check(3)
    Truncation(min_p=1.0, typical_p=1.0, epsilon_cutoff=0.999, eta_cutoff=0.999).check()

    # RowSampling carries it as grammar_state is carried: an attribute, not a field
    assert [f.name for f in dataclasses.fields(RowSampling)] == ["temperature", "top_k", "top_p", "repetition_penalty", "eos_id",
                                                                 "max_new_tokens", "seed", "stream", "logit_bias", "min_new_tokens"]
    row = RowSampling(0.9, 0, truncation=t)
    assert row.truncation is t and row.grammar_state is None
    assert dataclasses.replace(row, seed=4).truncation is t and dataclasses.replace(row, truncation=None).truncation is None
    assert RowSampling().truncation is None
    row.check(0, 100)
    with pytest.raises(ValueError, match="row 2: min_p"):
        RowSampling(truncation=Truncation(min_p=2.0)).check(2, 100)
    with pytest.raises(ValueError, match="row 1: truncation"):
        RowSampling(truncation=dict(min_p=0.1)).check(1, 100)

    assert pack_truncation([RowSampling(), RowSampling(grammar_state=1)]) is None
    recs = pack_truncation([RowSampling(), RowSampling(truncation=Truncation(epsilon_cutoff=3e-4)), RowSampling(truncation=Truncation())])
    assert len(recs) == 3 and recs[1].epsilon_cutoff == np.float32(3e-4)
    assert [(q.min_p, q.typical_p, q.epsilon_cutoff, q.eta_cutoff) for q in (recs[0], recs[2])] == [(0, 0, 0, 0)] * 2
    with pytest.raises(ValueError, match="row 1: eta_cutoff"):
        pack_truncation([RowSampling(), RowSampling(truncation=Truncation(eta_cutoff=-1.0))])


def test_header_prototypes_and_record_layout():
    import ctypes as C
    from mgea import _lib
    hdr = open(os.path.join(ROOT, "include", "mgea.h")).read()
    for name in ("mgea_decoder_generate_rows_truncated", "mgea_op_sample_rows_truncated", "mgea_decoder_truncation_info"):
        assert name + "(" in hdr and name in _lib.PROTOTYPES, name
    assert "float min_p, typical_p, epsilon_cutoff, eta_cutoff;" in hdr
    assert C.sizeof(_lib.RowTruncation) == 16 and C.sizeof(_lib.RowSampler) == 40
    sched, trunc = (_lib.PROTOTYPES[f"mgea_decoder_generate_rows_{n}"][1] for n in ("scheduled", "truncated"))
    assert trunc[:len(sched) - 1] == sched[:-1] and trunc[-2:] == [C.POINTER(_lib.RowTruncation), C.c_void_p]


def test_surface_keywords():
    import inspect
    import api_shim
    import generate_music.generate as gen
    from mgea.serve import RequestBatcher
    four = ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"]
    for f in (gen.sample_kvcache_truncated, gen.generate_sequence_truncated, gen.generate_batch_truncated, gen.sample_kvcache_grammar,
              gen.generate_batch_grammar, gen.generate_requests, gen.generate_best_of, gen.sample_kvcache_guided,
              gen.generate_requests_guided, gen.sample_kvcache_transitions, gen.generate_requests_transitions, RequestBatcher.submit,
              api_shim.create_truncated_app, api_shim.create_windowed_app, api_shim.create_grammar_app, api_shim.create_best_of_app,
              api_shim.create_guided_app, api_shim.create_transition_app):
        sig = inspect.signature(f).parameters
        assert all(n in sig and sig[n].default is None for n in four), f.__name__
    # the truncated variants extend the grammar ones, which keep their own arguments in front
    for new, old in ((gen.sample_kvcache_truncated, gen.sample_kvcache_grammar), (gen.generate_batch_truncated, gen.generate_batch_grammar)):
        assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters)
    with pytest.raises(ValueError, match="typical_p"):
        api_shim.create_truncated_app(None, 64, typical_p=1.5)
    with pytest.raises(ValueError, match="min_p"):
        api_shim.create_grammar_app(None, 64, min_p=-0.5)
    assert gen._per_prompt([0.1, None], 2, "min_p") == [0.1, None]


# ---------------------------------------------------------------------------------------------------------- the plan
def test_trunc_plan_native(tmp_path):
    """tests/native/trunc_plan_test.cpp: the refusals, truncated => form >= BIASED, NULL / all-off records => the plan there was,
    StepKind inequality.  A stand-alone host program; with AddressSanitizer and UBSan where there is no GPU."""
    exe = str(tmp_path / "trunc_plan_test")
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *san,
                           os.path.join(ROOT, "tests", "native", "trunc_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "trunc_plan ok" and r.stderr == "", r.stdout + r.stderr
