"""Lifetimes of the native handles' device buffers: handles that are created and destroyed in a row, the decoder's workspace and
its fp16-prefill buffers regrowing under a live handle, and device memory coming back at destroy.  The failure paths of the
allocations are covered on the CPU (test_devmem_host.py); nothing here provokes one."""
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
