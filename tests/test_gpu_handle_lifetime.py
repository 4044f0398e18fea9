"""Lifetimes of the native handles' resources: handles that are created and destroyed in a row, the decoder's workspace and
its fp16-prefill buffers regrowing under a live handle, device memory coming back at destroy, the step-graph cache filled past its
capacity, and an engine closed with unread profile records.  The failure paths of the allocations and the cache's rules one by one
are covered on the CPU (test_devmem_host.py); nothing here provokes a failure."""
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROMPTS = [[1, 5, 14], [1, 7, 20, 33, 34], [2, 9]]


@pytest.fixture(scope="module")
def small_sd():
    return synth.decoder_state_dict(71, 128, 128, 256, 2, d_ff=512)


def small_engine(sd, **kw):
    from mgea.decoder import DecoderEngine
    return DecoderEngine(sd, n_head=4, max_batch=4, max_ctx=128, device=DEV, **kw)


def greedy(eng, steps=8):
    return eng.generate(PROMPTS, steps, temperature=1.0, top_k=1).cpu().tolist()


def test_decoder_recreate_gives_the_same_ids(small_sd):
    keep = small_engine(small_sd)
    want = greedy(keep)
    for _ in range(3):
        eng = small_engine(small_sd)
        got = greedy(eng)
        eng.close()
        assert got == want
    assert greedy(keep) == want   # the handle that stayed alive is untouched by its neighbours' lifetimes
    keep.close()


def test_workspace_regrowth_drops_the_graphs_and_keeps_the_results(small_sd):
    eng = small_engine(small_sd)
    ids = greedy(eng)
    assert eng.stats()["graphs_cached"] > 0
    idx = torch.from_numpy(synth.integers(72, "regrow", (4, 40), 0, 128))
    got = eng.reset_and_prefill(idx).cpu()          # 160 rows: more than the 64 the workspace starts with
    assert eng.stats()["graphs_cached"] == 0        # the captured pointers went with the old workspace
    fresh = small_engine(small_sd)
    want = fresh.reset_and_prefill(idx).cpu()
    fresh.close()
    assert torch.equal(got, want)
    assert greedy(eng) == ids
    assert eng.stats()["graphs_cached"] > 0
    eng.close()


def test_fp16_prefill_regrowth_and_refresh(tune):
    from mgea.decoder import DecoderEngine
    tune("decoder_prefill16", 2)
    sd = synth.decoder_state_dict(73, 256, 256, 512, 1, d_ff=512)

    def engine():
        return DecoderEngine(sd, n_head=8, max_batch=8, max_ctx=256, device=DEV, dtype="f16")
    idx4 = torch.from_numpy(synth.integers(74, "p16a", (4, 256), 0, 256))
    idx8 = torch.from_numpy(synth.integers(74, "p16b", (8, 256), 0, 256))
    eng = engine()
    eng.reset_and_prefill(idx4, want_logits=False)   # (1024 rows x 256 columns are too few tiles for this path's LM-head GEMM: cache fill only)
    assert eng.stats()["prefill16_forwards"] == 1
    got = eng.reset_and_prefill(idx8).cpu()         # twice the rows: the activations regrow, the matrices stay
    assert eng.stats()["prefill16_forwards"] == 2
    fresh = engine()
    want = fresh.reset_and_prefill(idx8).cpu()
    assert fresh.stats()["prefill16_forwards"] == 1
    fresh.close()
    assert torch.equal(got, want)
    eng.refresh_weights()                           # same arena: the matrices are folded again into the buffers that are kept
    again = eng.reset_and_prefill(idx8).cpu()
    assert eng.stats()["prefill16_forwards"] == 3
    assert torch.equal(again, want)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bert_recreate_gives_the_same_logits(dtype):
    from mgea.bert import BertEngine
    bsd = synth.distilbert_state_dict(75, 200, 128, 128, 2, 256)
    ids, mask = synth.bert_inputs(76, 4, 128, 200, min_len=8)
    outs = []
    for _ in range(2):
        eng = BertEngine(bsd, n_heads=2, max_tokens=512, device=DEV, dtype=dtype)
        logits, _ = eng.forward(torch.from_numpy(ids), torch.from_numpy(mask))
        outs.append(logits.cpu())
        eng.close()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_destroy_returns_device_memory():
    """8 create - generate - close cycles of an engine whose KV pool is 256 MiB may cost at most ONE pool of free device memory
    (allocator slack); a handle that leaked only its pool would cost eight."""
    from mgea.decoder import DecoderEngine
    sd = synth.decoder_state_dict(77, 128, 64, 256, 2, d_ff=512)
    pool = 64 * 1024 * 2 * 256 * 2 * 4   # max_batch * max_ctx * n_layer * d_model * (K, V) * sizeof(float), as mgea_decoder_create sizes it
    assert pool == 256 << 20
    shared = {}

    def cycle():
        eng = DecoderEngine(sd if not shared else None, n_head=4, max_batch=64, max_ctx=1024, device=DEV, **shared)
        if not shared:   # later cycles borrow the first one's arena: what is measured is the handles' own memory
            shared.update(arena=eng.arena, geometry=eng.cfg_dict())
        ids = eng.generate(PROMPTS, 2, temperature=1.0, top_k=1).cpu()
        eng.close()
        return ids
    want = cycle()   # warm-up: code objects, torch's caching allocator
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(8):
        assert torch.equal(cycle(), want)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f"free device memory before {free0} after {free1}: dropped by {free0 - free1} bytes (bound {pool})")
    assert free0 - free1 <= pool


def tiny_engine():
    """d_model 256: the smallest geometry that takes the fused, graph-replayed path"""
    from mgea.decoder import DecoderEngine
    return DecoderEngine(synth.decoder_state_dict(78, 128, 64, 256, 1, d_ff=512), n_head=4, max_batch=10, max_ctx=64, device=DEV)


def test_step_graph_cache_evicts_the_least_recently_used(tune):
    """20 configurations x (1-step, 8-step graph) = 40 keys against the cache's 36: the first two configurations' graphs are evicted,
    a configuration that comes back is captured again at the cost of the oldest one left, and the ids never change."""
    tune("decoder_graph_steps", 8)
    eng = tiny_engine()
    configs = [(B, top_k) for B in range(1, 11) for top_k in (1, 50)]   # greedy, then sampled: two step forms per batch size

    def run(i):
        B, top_k = configs[i]
        prompts = [[1 + b, 5 + 2 * b, 14 + 3 * b] for b in range(B)]
        return eng.generate(prompts, 8, temperature=1.0, top_k=top_k, seed=79).cpu().tolist()

    def counts():
        st = eng.stats()
        return st["graph_instantiates"], st["graphs_cached"]

    first = []
    for i in range(20):
        first.append(run(i))
        inst, cached = counts()
        assert inst == 2 * (i + 1) and cached == min(2 * (i + 1), 36), f"after configuration {i + 1}: {inst} instantiated, {cached} cached"
    assert counts() == (40, 36)
    assert run(19) == first[19] and counts() == (40, 36)   # the last one: cached
    assert run(0) == first[0] and counts() == (42, 36)     # the first one was evicted: captured again, in the place of the third's graphs
    assert run(3) == first[3] and counts() == (42, 36)     # the fourth: never touched by an eviction
    assert run(2) == first[2] and counts() == (44, 36)     # the third: evicted a moment ago
    eng.close()


def test_unread_profile_records_go_with_the_engine():
    prompts = [[1, 5, 14], [2, 9, 4]]

    def ids(eng):
        return eng.generate(prompts, 4, temperature=1.0, top_k=1).cpu().tolist()
    plain = tiny_engine()
    want = ids(plain)
    plain.close()
    eng = tiny_engine()
    eng.profile(1)           # every step eagerly, an event pair around each launch
    assert ids(eng) == want
    eng.close()              # ... and nobody reads them
    eng = tiny_engine()
    assert ids(eng) == want
    eng.profile(1)
    assert ids(eng) == want
    eng.profile(0)
    rec = eng.profile_read()
    assert sum(r["launches"] for r in rec.values()) > 0 and all(r["ms"] >= 0.0 for r in rec.values())
    assert sum(r["launches"] for r in eng.profile_read().values()) == 0   # one read takes every record
    assert ids(eng) == want
    eng.close()
