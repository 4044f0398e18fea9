"""Per-row logit bias and min_new_tokens, host side (no GPU): the key / vocabulary constraints, the packing and validity checks of
the Python layer, the mgea_row_logits layout and the host checks of the C ABI, and how generate_requests, RequestBatcher.submit and
the endpoint hand the values on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf

PC = {"C": 0, "C#": 1, "D": 2, "E-": 3, "E": 4, "F": 5, "F#": 6, "G": 7, "G#": 8, "A": 9, "B-": 10, "B": 11}


def pcs(*names):
    return {PC[n] for n in names}


# ---------------------------------------------------------------------------------------------------------- constraints
@pytest.mark.parametrize("spellings, want", [
    (("D Major", "[KEY_SIGNATURE] D major"), pcs("D", "E", "F#", "G", "A", "B", "C#")),
    (("B♭ Major", "[KEY_SIGNATURE] B- major", "Bb major"), pcs("B-", "C", "D", "E-", "F", "G", "A")),
    (("E♭ Major", "[KEY_SIGNATURE] E- major"), pcs("E-", "F", "G", "G#", "B-", "C", "D")),
    (("C# Minor", "[KEY_SIGNATURE] C# minor", "C♯ Minor"), pcs("C#", "E-", "E", "F#", "G#", "A", "B")),
    (("G# Minor", "[KEY_SIGNATURE] G# minor"), pcs("G#", "B-", "B", "C#", "E-", "E", "F#"))])
def test_scale_pitch_classes(spellings, want):
    from generate_music.constraints import scale_pitch_classes
    assert len(want) == 7
    for s in spellings:
        assert scale_pitch_classes(s) == want, s


def test_scale_pitch_classes_rejects_what_is_no_key():
    from generate_music.constraints import scale_pitch_classes
    for bad in ("D", "H Major", "D lydian", "[KEY_SIGNATURE] unknown", ""):
        with pytest.raises(ValueError):
            scale_pitch_classes(bad)


def test_keys_of_the_lookup_table_all_parse():
    """every key EATS.get_music_params can return, through normalize_key_signature as the endpoint does it"""
    import csv
    import generate_music.generate as gen
    from generate_music.constraints import scale_pitch_classes
    path = os.path.join(ROOT, "music-generation-emotion-adaptive_amd", "emotion_analysis", "lookup_table.csv")
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.DictReader(f))
    col = [c for c in rows[0] if c.strip().lower() in ("key", "key_signature", "key signature")]
    assert col, list(rows[0])
    keys = {r[col[0]] for r in rows}
    assert keys
    for k in keys:
        assert len(scale_pitch_classes(gen.normalize_key_signature(k))) == 7, k


def test_classify_vocab_and_bias_on_the_synthetic_vocabulary():
    from generate_music import constraints
    from generate_music.midi import note_name_to_number, note_re
    from mgea import synth
    vocab = synth.decoder_vocab(8324, with_eos=True)
    cls = constraints.classify_vocab(vocab)
    assert cls["eos"] == vocab["[END_SEQUENCE]"]
    assert cls["instruments"] == sorted(i for t, i in vocab.items() if t.startswith("[INSTRUMENT]")) and len(cls["instruments"]) == 3
    assert len(cls["notes"]) + len(cls["instruments"]) + len(cls["control"]) + 1 == 8324
    assert vocab["[PAD]"] in cls["control"] and vocab["[BPM] 120"] in cls["control"] and vocab["[KEY_SIGNATURE] D major"] in cls["control"]
    for t, i in vocab.items():
        m = note_re.match(t)
        assert (i in cls["notes"]) == bool(m)
        if m:
            assert cls["notes"][i] == note_name_to_number(m.group(1)) % 12

    plain = constraints.logit_bias(vocab)
    assert plain.dtype == np.float32 and plain.shape == (8324,)
    assert np.all(plain[cls["control"]] == NINF)
    keep = sorted(cls["notes"]) + cls["instruments"] + [cls["eos"]]
    assert np.all(plain[keep] == 0) and np.isinf(plain).sum() == len(cls["control"])

    scale = constraints.scale_pitch_classes("E♭ Major")
    inside = [i for i, pc in cls["notes"].items() if pc in scale]
    outside = [i for i, pc in cls["notes"].items() if pc not in scale]
    assert inside and outside
    hard = constraints.logit_bias(vocab, key="E♭ Major")
    assert np.all(hard[cls["control"]] == NINF) and np.all(hard[outside] == NINF)
    assert np.all(hard[inside] == 0) and np.all(hard[cls["instruments"]] == 0) and hard[cls["eos"]] == 0
    soft = constraints.logit_bias(vocab, key="[KEY_SIGNATURE] E- major", out_of_scale=-4.0)
    assert np.all(soft[outside] == -4.0) and np.all(soft[inside] == 0) and np.all(soft[cls["control"]] == NINF)
    free = constraints.logit_bias(vocab, key="E♭ Major", notes_only=False, out_of_scale=-2.5)
    assert np.all(free[cls["control"]] == 0) and np.all(free[outside] == -2.5)
    for bad in (math.inf, math.nan):
        with pytest.raises(ValueError):
            constraints.logit_bias(vocab, key="D Major", out_of_scale=bad)


def test_bias_with_nothing_admissible_is_an_error():
    from generate_music import constraints
    only_control = {"[PAD]": 0, "[START_SEQUENCE]": 1, "[END_SEQUENCE]": 2, "[BPM] 120": 3}
    with pytest.raises(ValueError, match="admissible"):
        constraints.logit_bias(only_control)
    one_note = dict(only_control)
    one_note["[NOTE] [PITCH:C#4] [START:0.0] [END:0.5] [DURATION:0.5]"] = 4
    assert np.isfinite(constraints.logit_bias(one_note, key="D Major")[4])      # C# is in D major
    with pytest.raises(ValueError, match="admissible"):
        constraints.logit_bias(one_note, key="C Major")                         # ... and not in C major


# ---------------------------------------------------------------------------------------------------------- packing and checks
def test_dict_to_dense_packing():
    from mgea.decoder import dense_logit_bias
    v = dense_logit_bias({3: -1.5, 0: NINF, 99: 2.0}, 100)
    assert v.dtype == np.float32 and v.shape == (100,)
    assert v[3] == -1.5 and v[0] == NINF and v[99] == 2.0 and np.count_nonzero(v) == 3
    assert dense_logit_bias(None, 100) is None
    host = dense_logit_bias(torch.arange(100, dtype=torch.float64), 100)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host[7] == 7
    for bad in ({100: 1.0}, {-1: 1.0}, np.zeros(99, np.float32), np.zeros((2, 100), np.float32)):
        with pytest.raises(ValueError):
            dense_logit_bias(bad, 100)


def test_row_sampling_keeps_its_positional_fields_and_gains_trailing_ones():
    import dataclasses
    from mgea.decoder import RowSampling
    names = [f.name for f in dataclasses.fields(RowSampling)]
    assert names[:8] == ["temperature", "top_k", "top_p", "repetition_penalty", "eos_id", "max_new_tokens", "seed", "stream"]
    assert names[8:] == ["logit_bias", "min_new_tokens"]
    r = RowSampling()
    assert r.logit_bias is None and r.min_new_tokens == 0


def _vec(n=100, **at):
    v = np.zeros(n, np.float32)
    for k, x in at.items():
        v[int(k[1:])] = x
    return v


@pytest.mark.parametrize("fields, what", [
    (dict(logit_bias=_vec(i5=math.nan)), "NaN"),
    (dict(logit_bias=_vec(i5=math.inf)), r"\+inf"),
    (dict(logit_bias=np.full(100, NINF, np.float32)), "bans every token"),
    (dict(logit_bias={i: NINF for i in range(100) if i != 9}, eos_id=9, min_new_tokens=3), "eos_id 9"),
    (dict(logit_bias={100: 0.0}), "outside"),
    (dict(logit_bias=np.zeros(99, np.float32)), "logit_bias must be"),
    (dict(min_new_tokens=-1), "min_new_tokens"),
    (dict(min_new_tokens=51), "min_new_tokens")])
def test_validity_rules_name_the_row(fields, what):
    from mgea.decoder import RowSampling, pack_row_logits, pack_rows
    rows = [RowSampling(), RowSampling(logit_bias={1: -1.0}), RowSampling(**fields)]
    with pytest.raises(ValueError, match=r"row 2: .*" + what):
        pack_rows(rows, 100, 50)
        pack_row_logits(rows, 100, "cpu")


def test_valid_rows_pack_and_share_uploads():
    from mgea._lib import RowLogits
    from mgea.decoder import RowSampling, pack_row_logits
    assert pack_row_logits([RowSampling(), RowSampling(top_k=1)], 100, "cpu") == (None, [])
    shared = _vec(i3=NINF)
    only_eos_left_but_no_min = {i: NINF for i in range(100) if i != 9}
    rows = [RowSampling(logit_bias=shared), RowSampling(), RowSampling(logit_bias=shared, min_new_tokens=4, eos_id=3),
            RowSampling(logit_bias=only_eos_left_but_no_min, eos_id=9), RowSampling(min_new_tokens=7)]
    recs, keep = pack_row_logits(rows, 100, "cpu")
    assert isinstance(recs[0], RowLogits) and len(recs) == 5 and len(keep) == 2
    assert recs[0].bias_dev == recs[2].bias_dev == keep[0].data_ptr() and recs[3].bias_dev == keep[1].data_ptr()
    assert recs[1].bias_dev is None and recs[4].bias_dev is None
    assert [r.min_new_tokens for r in recs] == [0, 0, 4, 0, 7] and all(r.reserved == 0 for r in recs)
    assert keep[0].dtype == torch.float32 and keep[0][3] == NINF and keep[1][9] == 0


# ---------------------------------------------------------------------------------------------------------- C ABI
def test_row_logits_struct_layout_and_new_symbols():
    from mgea import _lib
    from mgea._lib import RowLogits
    assert C.sizeof(RowLogits) == 16
    assert {n: getattr(RowLogits, n).offset for n, _ in RowLogits._fields_} == dict(bias_dev=0, min_new_tokens=8, reserved=12)
    with open(os.path.join(ROOT, "include", "mgea.h")) as f:
        hdr = f.read()
    body = hdr[hdr.index("typedef struct mgea_row_logits {"):hdr.index("} mgea_row_logits;")]
    pos = [re.search(r"\b%s;" % n, body).start() for n, _ in RowLogits._fields_]
    assert pos == sorted(pos), "field order differs from include/mgea.h"
    for name in ("mgea_decoder_generate_rows_biased", "mgea_op_sample_rows_biased"):
        assert name + "(" in hdr, name
        assert name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["mgea_decoder_generate_rows_biased"][1][6]._type_ is _lib.RowSampler
    assert _lib.PROTOTYPES["mgea_decoder_generate_rows_biased"][1][7]._type_ is RowLogits
    assert _lib.PROTOTYPES["mgea_op_sample_rows_biased"][1][5]._type_ is RowLogits
    # the existing record is untouched
    assert C.sizeof(_lib.RowSampler) == 40


def _rec(**kw):
    from mgea._lib import RowSampler
    base = dict(temperature=1.0, top_k=50, top_p=0.0, repetition_penalty=1.0, eos_id=-1, max_new_tokens=0, seed=1, stream=0, reserved=0)
    base.update(kw)
    return RowSampler(**base)


@pytest.mark.parametrize("bad, what", [(dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=11), "min_new_tokens"),
                                       (dict(reserved=1), "reserved")])
def test_c_abi_checks_the_logits_records_on_the_host(bad, what):
    """The record checks run before any device work: no GPU is needed to see MGEA_EINVAL naming the row."""
    from mgea import _lib
    lib = _lib.load()
    recs = (_lib.RowSampler * 3)(_rec(), _rec(), _rec())
    fake = C.c_void_p(16)   # never dereferenced: the calls fail in their host checks
    lrecs = (_lib.RowLogits * 3)(_lib.RowLogits(16, 2, 0), _lib.RowLogits(None, 0, 0), _lib.RowLogits(16, **bad))
    # the engine call looks at the records before it looks at its handle: n_steps = 10 bounds min_new_tokens here
    assert lib.mgea_decoder_generate_rows_biased(None, fake, None, 3, 4, 10, recs, lrecs, fake, None) == _lib.EINVAL
    msg = _lib.last_error()
    assert "row 2" in msg and what in msg
    good = (_lib.RowLogits * 3)(_lib.RowLogits(16, 10, 0), _lib.RowLogits(None, 0, 0), _lib.RowLogits(16, 0, 0))
    assert lib.mgea_decoder_generate_rows_biased(None, fake, None, 3, 4, 10, recs, good, fake, None) == _lib.EINVAL
    assert "NULL" in _lib.last_error()            # good records: only the missing handle is left to refuse
    if what != "min_new_tokens" or bad["min_new_tokens"] < 0:   # the op has no n_steps to bound min_new_tokens with
        assert lib.mgea_op_sample_rows_biased(fake, 3, 100, recs, None, lrecs, 0, fake, None, None) == _lib.EINVAL
        msg = _lib.last_error()
        assert "row 2" in msg and what in msg
    # a bad sampler record is still found first, whatever the logits records say
    recs_bad = (_lib.RowSampler * 3)(_rec(), _rec(temperature=0.0), _rec())
    assert lib.mgea_op_sample_rows_biased(fake, 3, 100, recs_bad, None, lrecs, 0, fake, None, None) == _lib.EINVAL
    assert "row 1" in _lib.last_error() and "temperature" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------------- generate_requests
class StubEngine:
    """What generate_requests needs of a DecoderEngine: max_batch, max_ctx, generate_rows(prompts, rows, n_steps)."""

    def __init__(self, vocab=64, max_batch=8, max_ctx=128):
        self.vocab, self.max_batch, self.max_ctx = vocab, max_batch, max_ctx
        self.calls = []

    def generate_rows(self, prompts, rows, n_steps=None):
        self.calls.append(dict(prompts=[list(p) for p in prompts], rows=list(rows), n_steps=n_steps))
        out = torch.full((len(prompts), n_steps), -1, dtype=torch.int32)
        for b, (p, r) in enumerate(zip(prompts, rows)):
            k = r.max_new_tokens or n_steps
            out[b, :k] = (torch.arange(k) + p[-1] + 1) % (self.vocab - 1)
        return out


def stub_model(vocab=64, **kw):
    import generate_music.generate as gen
    from mgea import synth
    gen.set_vocab(synth.decoder_vocab(vocab, with_eos=True))
    m = gen.GPTWithKV(vocab, 128, 64, 2, 1)
    m.engine = StubEngine(vocab, **kw)
    return m, gen


def test_generate_requests_puts_bias_and_min_new_into_the_right_records():
    m, gen = stub_model()
    names = list(gen.tok2id)
    prompts = [names[3:6], names[10:14], names[20:21], names[30:33]]
    b1, b3 = {5: NINF}, np.zeros(64, np.float32)
    out = gen.generate_requests(m, prompts, max_len=[9, 12, 3, 1], top_k=1, seed=0, logit_bias=[None, b1, b3, b1],
                                min_new_tokens=[0, 5, 7, 2])
    call, = m.engine.calls                       # prompt 3 has no budget: no row
    rows = call["rows"]
    assert len(rows) == 3 and call["n_steps"] == 8
    assert rows[0].logit_bias is None and rows[1].logit_bias is b1 and rows[2].logit_bias is b3
    assert [r.min_new_tokens for r in rows] == [0, 5, 2]          # capped at the row's budget (3 - 1 = 2)
    assert [len(o) for o in out] == [9, 12, 3, 3]
    # one value for every prompt
    m.engine.calls.clear()
    gen.generate_requests(m, prompts[:2], max_len=10, top_k=1, seed=0, logit_bias=b3, min_new_tokens=4)
    rows = m.engine.calls[0]["rows"]
    assert all(r.logit_bias is b3 and r.min_new_tokens == 4 for r in rows)
    with pytest.raises(ValueError, match="logit_bias"):
        gen.generate_requests(m, prompts[:2], 10, logit_bias=[b1])
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen.generate_requests(m, prompts[:2], 10, min_new_tokens=[0, -2])


def test_generate_requests_is_unchanged_without_them():
    from mgea.decoder import RowSampling
    m, gen = stub_model()
    names = list(gen.tok2id)
    gen.generate_requests(m, [names[3:6], names[10:14]], max_len=[9, 12], temperature=0.7, top_k=[1, 50], seed=[1, 2])
    call, = m.engine.calls
    eos = gen.tok2id["[END_SEQUENCE]"]
    assert call["rows"] == [RowSampling(0.7, 1, None, None, eos, 6, 1, 0), RowSampling(0.7, 50, None, None, eos, 8, 2, 0)]
    assert all(r.logit_bias is None and r.min_new_tokens == 0 for r in call["rows"])


def test_biased_entry_points_call_generate_biased_only_when_something_is_set():
    m, gen = stub_model()
    names = list(gen.tok2id)
    seen = []

    def make(which):
        def generate(prompts, n_steps, **kw):
            seen.append((which, kw))
            return torch.full((len(prompts), n_steps), 40, dtype=torch.int32)
        return generate
    m.engine.generate, m.engine.generate_biased = make("generate"), make("generate_biased")
    a = gen.sample_kvcache(m, names[3:6], 10, top_k=1, seed=0)
    b = gen.sample_kvcache_biased(m, names[3:6], 10, top_k=1, seed=0)
    assert a == b and [w for w, _ in seen] == ["generate", "generate"] and seen[0][1] == seen[1][1]
    assert "logit_bias" not in seen[-1][1] and "min_new_tokens" not in seen[-1][1]
    bias = {5: NINF}
    gen.sample_kvcache_biased(m, names[3:6], 10, top_k=1, seed=0, logit_bias=bias, min_new_tokens=50)
    which, kw = seen[-1]
    assert which == "generate_biased" and kw["logit_bias"] is bias and kw["min_new_tokens"] == 7   # capped at the 7 steps there are
    gen.generate_batch_biased(m, [names[3:6], names[6:8]], 10, top_k=1, seed=0, min_new_tokens=3)
    which, kw = seen[-1]
    assert which == "generate_biased" and kw["logit_bias"] is None and kw["min_new_tokens"] == 3
    gen.generate_batch(m, [names[3:6], names[6:8]], 10, top_k=1, seed=0)
    assert seen[-1][0] == "generate"


def test_existing_entry_points_keep_their_parameter_lists():
    """the bias arrives through new names: generate_biased, sample_biased, sample_kvcache_biased, generate_sequence_biased, generate_batch_biased,
    create_constrained_app"""
    import inspect
    import api_shim
    import generate_music.generate as gen
    from mgea import ops
    from mgea.decoder import DecoderEngine

    def params(f):
        return list(inspect.signature(f).parameters)
    for old, new, extra in ((gen.sample_kvcache, gen.sample_kvcache_biased, ["logit_bias", "min_new_tokens"]),
                            (gen.generate_batch, gen.generate_batch_biased, ["logit_bias", "min_new_tokens"]),
                            (gen.generate_sequence, gen.generate_sequence_biased, ["logit_bias", "min_new_tokens"]),
                            (DecoderEngine.generate, DecoderEngine.generate_biased, ["logit_bias", "min_new_tokens", "check_bias"]),
                            (ops.sample, ops.sample_biased, ["logit_bias"]),
                            (api_shim.create_app, api_shim.create_constrained_app, ["constrain", "out_of_scale_bias", "min_new_tokens"])):
        assert params(new) == params(old) + extra, new.__name__
    assert params(api_shim.create_batched_app)[-3:] == ["constrain", "out_of_scale_bias", "min_new_tokens"]


# ---------------------------------------------------------------------------------------------------------- serving
def test_submit_validates_in_the_callers_thread():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    b = RequestBatcher(m, autostart=False)
    try:
        with pytest.raises(ValueError, match="NaN"):
            b.submit(names[3:6], 10, logit_bias=_vec(64, i2=math.nan))
        with pytest.raises(ValueError, match="bans every token"):
            b.submit(names[3:6], 10, logit_bias=np.full(64, NINF, np.float32))
        with pytest.raises(ValueError, match="outside"):
            b.submit(names[3:6], 10, logit_bias={64: 1.0})
        with pytest.raises(ValueError, match="min_new_tokens"):
            b.submit(names[3:6], 10, min_new_tokens=-1)
        eos = gen.tok2id["[END_SEQUENCE]"]
        with pytest.raises(ValueError, match="eos_id"):
            b.submit(names[3:6], 10, logit_bias={i: NINF for i in range(64) if i != eos}, min_new_tokens=2)
        assert not b._queue
        gen.tok2id["[EXTRA]"] = 200                   # the vector is sized by the engine's vocabulary, not by the names there are
        try:
            with pytest.raises(ValueError, match="outside"):
                b.submit(names[3:6], 10, logit_bias={64: 1.0})
            with pytest.raises(ValueError, match="logit_bias must be"):
                b.submit(names[3:6], 10, logit_bias=np.zeros(65, np.float32))
        finally:
            del gen.tok2id["[EXTRA]"]
        fut = b.submit(names[3:6], 10, seed=1, logit_bias={5: NINF}, min_new_tokens=2)
        req, = b._queue
        assert req.kwargs["min_new_tokens"] == 2 and req.kwargs["logit_bias"].shape == (64,) and req.kwargs["logit_bias"][5] == NINF
        assert not fut.done()
    finally:
        b.close()


def test_batcher_serves_a_biased_request_through_generate_requests():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    b = RequestBatcher(m)
    try:
        out = b.submit(names[3:6], 10, top_k=1, seed=1, logit_bias={5: NINF}, min_new_tokens=2).result(timeout=30)
    finally:
        b.close()
    assert len(out) == 10
    row, = m.engine.calls[0]["rows"]
    assert row.min_new_tokens == 2 and row.logit_bias[5] == NINF and row.max_new_tokens == 7


def test_shim_rejects_bad_constraint_options_at_creation():
    import api_shim
    with pytest.raises(ValueError, match="constrain"):
        api_shim.create_constrained_app(None, 64, constrain="bogus")
    with pytest.raises(ValueError, match="constrain"):
        api_shim.create_batched_app(None, 64, constrain="bogus")
    with pytest.raises(ValueError, match="out_of_scale_bias"):
        api_shim.create_constrained_app(None, 64, constrain="scale", out_of_scale_bias=math.nan)
    with pytest.raises(ValueError, match="out_of_scale_bias"):
        api_shim.create_constrained_app(None, 64, constrain="scale", out_of_scale_bias=math.inf)
    with pytest.raises(ValueError, match="min_new_tokens"):
        api_shim.create_constrained_app(None, 64, min_new_tokens=-3)
