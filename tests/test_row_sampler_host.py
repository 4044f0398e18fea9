"""Per-row sampler records, host side (no GPU): the mgea_row_sampler layout and its Python packing, the checks of the Python layer
and of the C ABI, and generate_requests' argument broadcasting and per-prompt budgets on a stub engine."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_sampler_struct_layout():
    from mgea._lib import RowSampler
    assert C.sizeof(RowSampler) == 40
    offs = {name: getattr(RowSampler, name).offset for name, _ in RowSampler._fields_}
    assert offs == dict(temperature=0, top_k=4, top_p=8, repetition_penalty=12, eos_id=16, max_new_tokens=20, seed=24, stream=32,
                        reserved=36)
    with open(os.path.join(ROOT, "include", "mgea.h")) as f:
        hdr = f.read()
    body = hdr[hdr.index("typedef struct mgea_row_sampler {"):hdr.index("} mgea_row_sampler;")]
    order = [n for n, _ in RowSampler._fields_]
    pos = [re.search(r"\b%s;" % n, body).start() for n in order]
    assert pos == sorted(pos), "field order differs from include/mgea.h"


def test_new_symbols_in_header_and_prototypes():
    from mgea import _lib
    with open(os.path.join(ROOT, "include", "mgea.h")) as f:
        hdr = f.read()
    for name in ("mgea_decoder_generate_rows", "mgea_op_sample_rows"):
        assert name + "(" in hdr, name
        assert name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["mgea_decoder_generate_rows"][1][6]._type_ is _lib.RowSampler
    assert _lib.PROTOTYPES["mgea_op_sample_rows"][1][3]._type_ is _lib.RowSampler


def test_record_packing_defaults_and_stream():
    from mgea.decoder import RowSampling, pack_rows
    rows = [RowSampling(), RowSampling(0.7, 1, 0.92, 1.1, eos_id=9, max_new_tokens=37, seed=-1, stream=5),
            RowSampling(top_k=None, seed=2 ** 64 + 3)]
    recs = pack_rows(rows, 100, 50)
    assert len(recs) == 3
    r0, r1, r2 = recs
    assert (r0.temperature, r0.top_k, r0.top_p, r0.repetition_penalty, r0.eos_id, r0.max_new_tokens, r0.seed, r0.stream) == \
        (1.0, 50, 0.0, 1.0, -1, 0, 0, 0)
    assert r1.top_k == 1 and abs(r1.temperature - 0.7) < 1e-7 and abs(r1.top_p - 0.92) < 1e-7 and abs(r1.repetition_penalty - 1.1) < 1e-7
    assert (r1.eos_id, r1.max_new_tokens, r1.seed, r1.stream, r1.reserved) == (9, 37, 2 ** 64 - 1, 5, 0)
    assert (r2.top_k, r2.seed, r2.stream) == (0, 3, 2)   # stream None = the row's index


@pytest.mark.parametrize("bad, what", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=1e-50), "temperature"), (dict(top_k=101), "top_k"), (dict(top_k=-1), "top_k"),
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
    (dict(max_new_tokens=51), "max_new_tokens"), (dict(max_new_tokens=-1), "max_new_tokens"), (dict(stream=2 ** 32), "stream")])
def test_python_checks_name_the_row(bad, what):
    from mgea.decoder import RowSampling, pack_rows
    rows = [RowSampling(), RowSampling(), RowSampling(**bad)]
    with pytest.raises(ValueError, match=r"row 2: .*" + what):
        pack_rows(rows, 100, 50)


def _rec(**kw):
    from mgea._lib import RowSampler
    base = dict(temperature=1.0, top_k=50, top_p=0.0, repetition_penalty=1.0, eos_id=-1, max_new_tokens=0, seed=1, stream=0,
                reserved=0)
    base.update(kw)
    return RowSampler(**base)


@pytest.mark.parametrize("bad, what", [(dict(temperature=0.0), "temperature"), (dict(temperature=float("inf")), "temperature"),
                                       (dict(top_k=101), "top_k"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
                                       (dict(repetition_penalty=float("nan")), "repetition_penalty")])
def test_c_abi_checks_every_record_on_the_host(bad, what):
    """The record checks run before any device work: no GPU is needed to see MGEA_EINVAL naming the row."""
    from mgea import _lib
    lib = _lib.load()
    recs = (_lib.RowSampler * 3)(_rec(), _rec(), _rec(**bad))
    fake = C.c_void_p(16)   # never dereferenced: the call fails in its host checks
    rc = lib.mgea_op_sample_rows(fake, 3, 100, recs, None, 0, fake, None, None)
    assert rc == _lib.EINVAL
    msg = _lib.last_error()
    assert "row 2" in msg and what in msg
    assert lib.mgea_decoder_generate_rows(None, fake, None, 3, 4, 10, recs, fake, None) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------------------- generate_requests
class StubEngine:
    """What generate_requests needs of a DecoderEngine: max_batch, max_ctx, generate_rows.  Row b's ids are its last prompt id + 1,
    + 2, ... for its budget, then -1."""

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


def test_generate_requests_broadcasts_and_budgets():
    m, gen = stub_model()
    names = list(gen.tok2id)
    prompts = [names[3:6], names[10:14], names[20:21]]
    out = gen.generate_requests(m, prompts, max_len=[9, 12, 5], temperature=0.7, top_k=[1, 50, 0], top_p=0.9, seed=[1, 2, 3],
                                repetition_penalty=[None, 1.1, 1.2])
    call, = m.engine.calls
    assert call["n_steps"] == 8 and call["prompts"] == [[gen.tok2id[t] for t in p] for p in prompts]
    rows = call["rows"]
    assert [r.max_new_tokens for r in rows] == [6, 8, 4]
    assert [r.top_k for r in rows] == [1, 50, 0] and all(r.temperature == 0.7 and r.top_p == 0.9 for r in rows)
    assert [r.repetition_penalty for r in rows] == [None, 1.1, 1.2] and [r.seed for r in rows] == [1, 2, 3]
    assert all(r.stream == 0 and r.eos_id == gen.tok2id["[END_SEQUENCE]"] for r in rows)
    for p, o, L in zip(prompts, out, (9, 12, 5)):
        assert o[:len(p)] == p and len(o) == L


def test_generate_requests_skips_spent_prompts_and_splits_batches():
    m, gen = stub_model(max_batch=2)
    names = list(gen.tok2id)
    prompts = [names[1:5], names[5:7], names[7:8], names[8:10], names[10:13]]
    out = gen.generate_requests(m, prompts, max_len=[4, 6, 3, 2, 10], top_k=1, seed=0)
    assert out[0] == prompts[0] and out[3] == prompts[3]           # nothing to generate: the prompt, no engine row
    assert [len(c["prompts"]) for c in m.engine.calls] == [2, 1]    # 3 live rows, max_batch 2
    assert [len(o) for o in out] == [4, 6, 3, 2, 10]


def test_generate_requests_argument_errors():
    m, gen = stub_model()
    names = list(gen.tok2id)
    with pytest.raises(ValueError, match="top_k"):
        gen.generate_requests(m, [names[1:3], names[3:5]], 10, top_k=[1, 2, 3])
    with pytest.raises(KeyError):
        gen.generate_requests(m, [names[1:3], ["no such token"]], 10)
    with pytest.raises(RuntimeError, match="max_len"):
        gen.generate_requests(m, [names[1:3]], 1000)
    assert not m.engine.calls


def test_generate_requests_draws_seeds_from_torch():
    m, gen = stub_model()
    names = list(gen.tok2id)
    torch.manual_seed(7)
    gen.generate_requests(m, [names[1:3], names[3:5]], 10, seed=[None, 5])
    torch.manual_seed(7)
    gen.generate_requests(m, [names[1:3], names[3:5]], 10, seed=[None, 5])
    a, b = ([r.seed for r in c["rows"]] for c in m.engine.calls)
    assert a == b and a[1] == 5
