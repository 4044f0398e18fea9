"""Request batching on the MI355X: ragged requests with their own budgets served by one generation against the oracle, and the
HTTP endpoint with batching on against the one-request-at-a-time endpoint."""
import random

import pytest
import torch

from mgea import synth
from parity_util import check_greedy_vs_oracle

pytestmark = pytest.mark.gpu


def test_ragged_requests_through_one_generation(golden):
    import generate_music.generate as gen
    from mgea.serve import RequestBatcher
    from oracle.decoder_ref import DecoderRef

    g = golden("decoder_S")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer, max_batch=8, max_ctx=96)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    names = list(gen.tok2id)
    prompts = [["[START_SEQUENCE]"] + names[40 + 7 * i:40 + 7 * i + n] for i, n in enumerate((2, 5, 3, 7, 1, 4))]
    max_lens = [40, 71, 23, 96, 96, 64]   # request 4: 2 + 94 tokens, past longest prompt + n_steps = 102 > max_ctx 96
    b = RequestBatcher(model, autostart=False)
    futs = [b.submit(p, max_len=L, top_k=1) for p, L in zip(prompts, max_lens)]
    b.start()
    outs = [f.result(timeout=300) for f in futs]
    b.close()
    assert b.stats()["rows_per_generation"] == [6]
    ref = DecoderRef(sd, n_head)
    eng = model.engine
    for i, (p, L, o) in enumerate(zip(prompts, max_lens, outs)):
        assert o[:len(p)] == p and len(o) == L
        ids = [gen.tok2id[t] for t in p]
        got = torch.tensor([[gen.tok2id[t] for t in o[len(p):]]], dtype=torch.int32)
        check_greedy_vs_oracle(eng, ref, [ids], L - len(p), f"batched request {i}", got=got)


def test_http_with_batching_matches_the_plain_endpoint(golden):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient
    import generate_music.generate as gen
    from api_shim import create_app, create_batched_app
    from emotion_analysis import inference
    from mgea.bert import BertEngine
    from mgea.tokenizer import WordPieceTokenizer

    g = golden("decoder_tiny8h")
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in g["cfg"])
    sd = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    gen.set_vocab(synth.decoder_vocab(vocab))
    model = gen.GPTWithKV(vocab, seq_len, d_model, n_head, n_layer)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + "i am walking down a road and see rainbow it is sunny . love life".split()
    vmap = {w: i for i, w in enumerate(dict.fromkeys(words))}
    bsd = synth.distilbert_state_dict(61, len(vmap), 64, 128, 2, 512)
    inference.configure(WordPieceTokenizer(vmap), BertEngine(bsd, n_heads=2, adapter=synth.lora_adapter(61, 128, 2), max_tokens=64))

    plain = create_app(model, seq_len=32, temperature=1.0, top_k=1)
    batched = create_batched_app(model, seq_len=32, temperature=1.0, top_k=1)
    assert plain.state.batcher is None and batched.state.batcher is not None
    for text in ("i am walking down a road and i see a rainbow. i love life.", "it is sunny"):
        kw = {"data": {"prompt": text}} if plain.state.prompt_in == "form" else {"params": {"prompt": text}}
        random.seed(11)
        want = TestClient(plain).post("/generate", **kw)
        random.seed(11)
        got = TestClient(batched).post("/generate", **kw)
        assert want.status_code == 200 and got.status_code == 200
        assert got.content == want.content
        for h in ("x-emotion", "x-prompt-tokens", "x-generated-tokens"):
            assert got.headers[h] == want.headers[h]
        assert got.headers["x-batch-rows"] == "1" and "x-batch-rows" not in want.headers
    batched.state.batcher.close()
    assert batched.state.batcher.stats()["rows_per_generation"] == [1, 1]
