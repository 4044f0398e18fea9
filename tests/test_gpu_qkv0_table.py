"""Layer 0's q | k | v from the per-token table (switch decoder_qkv0_table; csrc/decoder_handle.h, "qkv0 table"): an engine created with the
switch on and one created with it off produce the same bits -- ids, log-probabilities, error flags -- in every step form, across a page
boundary, for rows that stop, with a full cache and on both decode paths (3..64 rows: MFMA kernels; 1..2 rows: dot products), and the
form is not taken where it must not be (more than 64 rows, absolute positions, fp16 engines, mgea_decoder_step)."""
import numpy as np
import pytest
import torch

from mgea import synth

pytestmark = pytest.mark.gpu
EOS = 2
FORMS = ("greedy", "sampled", "penalized", "biased")
_SD = {}


def state_dict(g):
    key = tuple(int(x) for x in g["cfg"])
    if key not in _SD:
        seed, vocab, seq_len, d_model, n_head, n_layer = key
        _SD[key] = synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer)
    return _SD[key]


def make(g, on, max_batch=8, max_ctx=None, **kw):
    """An engine with the switch latched at `on` (read when the handle is created)"""
    from mgea import _lib
    from mgea.decoder import DecoderEngine
    old = _lib.tune_set("decoder_qkv0_table", int(on))
    try:
        return DecoderEngine(state_dict(g), n_head=int(g["cfg"][4]), max_batch=max_batch, max_ctx=max_ctx or int(g["cfg"][2]), **kw)
    finally:
        _lib.tune_set("decoder_qkv0_table", old)


def pair(g, **kw):
    return make(g, 1, **kw), make(g, 0, **kw)


def table_bytes(eng):
    return eng.vocab * 3 * eng.d_model * 4


def rand_prompts(rng, B, vocab, lo, hi):
    return [rng.integers(0, vocab, int(rng.integers(lo, hi + 1))).tolist() for _ in range(B)]


def same_scored(a, b):
    return torch.equal(a.ids, b.ids) and torch.equal(a.logprobs, b.logprobs) and torch.equal(a.choice_logprobs, b.choice_logprobs)


@pytest.mark.parametrize("B", [3, 16, 24, 64])
def test_bitwise_identity_through_a_page_boundary(golden, B):
    """Ragged prompts of 58-63 tokens, 12 greedy steps: the rows cross position 64 (one KV page) at different steps.
    3 and 16 rows run the in-projection on 16-row tiles, 24 and 64 on the 32-row tiles the table's 64-row chunks were built with."""
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    on, off = pair(g, max_batch=64, max_ctx=128)
    rng = np.random.default_rng(100 + B)
    prompts = [rng.integers(0, on.vocab, 58 + b % 6).tolist() for b in range(B)]   # row b crosses the boundary at step 6 - b % 6
    rows = [RowSampling(top_k=1) for _ in prompts]
    a, b = on.generate_scored(prompts, rows, 12), off.generate_scored(prompts, rows, 12)
    assert int(a.ids.min()) >= 0 and same_scored(a, b)
    assert torch.equal(on.generate(prompts, 12, top_k=1), off.generate(prompts, 12, top_k=1))
    assert on.stats()["qkv0_table_bytes"] == table_bytes(on) and off.stats()["qkv0_table_bytes"] == 0
    on.close(), off.close()


def test_golden_greedy_ids_with_the_table(golden):
    g = golden("decoder_S")
    on = make(g, 1)
    prompts = [g[f"prompt{i}"].tolist() for i in range(4)]
    out = on.generate(prompts, 48, top_k=1).cpu()
    assert on.stats()["graph_nodes"] == 31
    for i, p in enumerate(prompts):
        assert p + out[i].tolist() == g[f"greedy{i}"].tolist(), f"row {i} diverged from the reference"
    on.close()


def form_rows(form, B, bias):
    from mgea.decoder import RowSampling
    if form == "greedy":
        return [RowSampling(top_k=1) for _ in range(B)]
    if form == "sampled":
        return [RowSampling(top_k=50, seed=7) for _ in range(B)]
    if form == "penalized":
        return [RowSampling(top_k=50, seed=7, repetition_penalty=1.2) for _ in range(B)]
    return [RowSampling(1.0, 50, None, 1.2, EOS, 0, 7, None, bias, 3) for _ in range(B)]


@pytest.mark.parametrize("scored", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_every_step_form_graphs_and_eager(golden, tune, form, scored):
    """40 steps of 3 rows as single-step graphs, as 8-step graphs and as eager launches (the profile stride forces them)."""
    g = golden("decoder_tiny8h")
    on, off = pair(g, max_batch=4)
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)]
    bias = (np.random.default_rng(5).standard_normal(on.vocab) * 2).astype(np.float32)
    rows = form_rows(form, 3, bias)

    def run(eng):
        if scored:
            r = eng.generate_scored(prompts, rows, 40)
            return torch.stack([r.ids.float(), r.logprobs, r.choice_logprobs]).cpu()
        return eng.generate_rows(prompts, rows, 40).cpu()

    want = None
    for mode in ("graph1", "graph8", "eager"):
        tune("decoder_graph_steps", 1 if mode == "graph1" else 8)
        for e in (on, off):
            e.profile(1 if mode == "eager" else 0)
        a, b = run(on), run(off)
        for e in (on, off):
            e.profile_read()
            e.profile(0)
        assert torch.equal(a, b), f"{form}, scored={scored}, {mode}: table and launch differ"
        want = a if want is None else want
        assert torch.equal(a, want), f"{form}, scored={scored}: {mode} differs from the single-step graphs"
    assert on.stats()["qkv0_table_bytes"] == table_bytes(on) and on.stats()["graph_nodes"] == off.stats()["graph_nodes"] - 1
    on.close(), off.close()


def test_rows_that_stop(golden):
    """One row meets its EOS id near step 5, the rows have budgets of their own, one forced id lies outside the vocabulary (clamped, error
    flag bit 0); then a second generation on the same handles: no q | k | v row of the first survives."""
    from mgea.decoder import RowSampling
    g = golden("decoder_tiny8h")
    on, off = pair(g, max_batch=4)
    V = on.vocab
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)] + [[7, 9, 11, 250, 3]]
    dry = off.generate(prompts, 12, top_k=1).cpu()
    eos = int(dry[1, 5])
    rows = [RowSampling(top_k=1, max_new_tokens=7), RowSampling(top_k=1, eos_id=eos, max_new_tokens=12),
            RowSampling(top_k=50, seed=3, max_new_tokens=12), RowSampling(top_k=1, max_new_tokens=9)]
    forced = torch.full((4, 12), -1, dtype=torch.int32)
    forced[3, 2] = V + 5
    outs = []
    for e in (on, off):
        r = e.generate_scored(prompts, rows, 12, force_ids=forced.cuda(), check_ids=False)
        outs.append((r, e.id_errors(raise_error=False)))
    (a, fa), (b, fb) = outs
    assert same_scored(a, b) and fa == fb == 1
    ids = a.ids.cpu()
    assert int(ids[3, 2]) == V - 1 and (ids[0, 7:] == -1).all() and (ids[3, 9:] == -1).all()
    stop = dry[1].tolist().index(eos)
    assert stop <= 5 and int(ids[1, stop]) == eos and (ids[1, stop + 1:] == -1).all()
    other = rand_prompts(np.random.default_rng(9), 4, V, 2, 6)
    assert torch.equal(on.generate_rows(other, rows, 12), off.generate_rows(other, rows, 12))
    assert torch.equal(on.generate(other, 12, top_k=1), off.generate(other, 12, top_k=1))
    on.close(), off.close()


def test_a_full_cache(golden):
    """max_ctx 128: every row generates until its two pages are full and is parked there"""
    from mgea.decoder import RowSampling
    g = golden("decoder_tiny8h")
    on, off = pair(g, max_batch=4, max_ctx=128)
    prompts = rand_prompts(np.random.default_rng(11), 3, on.vocab, 40, 47)
    prompts[0] = prompts[0][:40]
    rows = [RowSampling(top_k=1, max_new_tokens=128 - len(p)) for p in prompts]
    a, b = on.generate_rows(prompts, rows).cpu(), off.generate_rows(prompts, rows).cpu()
    assert torch.equal(a, b)
    for i, p in enumerate(prompts):
        assert int((a[i] >= 0).sum()) == 128 - len(p)
    assert torch.equal(on.context_lengths(), off.context_lengths())
    on.close(), off.close()


def test_beyond_64_rows_keeps_the_launch(golden):
    g = golden("decoder_S")
    on = make(g, 1, max_batch=100, max_ctx=64)
    prompts = synth.integers(7, "p100", (100, 5), 0, on.vocab).tolist()
    big = on.generate(prompts, 4, top_k=1).cpu()
    st = on.stats()
    assert st["graph_nodes"] == 32 and st["qkv0_table_bytes"] == 0
    small = on.generate(prompts[:3], 4, top_k=1).cpu()
    assert on.stats()["graph_nodes"] == 31 and torch.equal(small, big[:3])
    on.close()


def test_absolute_positions_keep_the_launch(golden):
    g = golden("decoder_S")
    on, off = pair(g, max_batch=4, max_ctx=64, pos_mode="absolute")
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)]
    a, b = on.generate(prompts, 12, top_k=1), off.generate(prompts, 12, top_k=1)
    assert torch.equal(a, b) and on.stats()["graph_nodes"] == 32 and on.stats()["qkv0_table_bytes"] == 0
    on.close(), off.close()


def test_f16_engines_have_no_table(golden):
    g = golden("decoder_tiny8h")
    on = make(g, 1, max_batch=4, dtype="f16")
    on.generate([g[f"prompt{i}"].tolist() for i in range(3)], 8, top_k=1)
    assert on.stats()["qkv0_table_bytes"] == 0
    on.close()


def test_step_after_generate_is_the_unprimed_step(golden):
    g = golden("decoder_tiny8h")
    on, off = pair(g, max_batch=4)
    prompts = [g[f"prompt{i}"].tolist() for i in range(3)]
    assert torch.equal(on.generate(prompts, 6, top_k=1), off.generate(prompts, 6, top_k=1))
    assert on.stats()["qkv0_table_bytes"] == table_bytes(on)
    samp = on.sampler(1.0, 1)
    idx = torch.tensor([[5, 6, 7, 8]] * 3)
    for e in (on, off):
        e.reset_and_prefill(idx, want_logits=False)
    for _ in range(3):
        (ia, la), (ib, lb) = on.step(None, samp, want_logits=True), off.step(None, samp, want_logits=True)
        assert torch.equal(ia, ib) and torch.equal(la, lb)
    on.close(), off.close()


def test_node_count_and_table_size(golden):
    g = golden("decoder_S")
    on, off = pair(g, max_batch=64, max_ctx=64)
    prompts = synth.integers(3, "p64", (64, 5), 0, on.vocab).tolist()
    assert torch.equal(on.generate(prompts, 9, top_k=1), off.generate(prompts, 9, top_k=1))
    assert on.stats()["graph_nodes"] == 31 and off.stats()["graph_nodes"] == 32
    assert on.stats()["qkv0_table_bytes"] == on.vocab * 3 * on.d_model * 4 == 8324 * 1536 * 4
    on.close(), off.close()


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_rows(golden, B):
    """The dot-product path and its own table: 120 steps (two pages), greedy and top-k 50"""
    from mgea.decoder import RowSampling
    g = golden("decoder_S")
    on, off = pair(g, max_batch=8, max_ctx=256)
    prompts = [g[f"prompt{i}"].tolist() for i in range(B)]
    for rows in ([RowSampling(top_k=1) for _ in prompts], [RowSampling(top_k=50, seed=11) for _ in prompts]):
        assert same_scored(on.generate_scored(prompts, rows, 120), off.generate_scored(prompts, rows, 120))
        assert torch.equal(on.generate_rows(prompts, rows, 120), off.generate_rows(prompts, rows, 120))
    assert on.stats()["graph_nodes"] == 31 and off.stats()["graph_nodes"] == 32
    assert on.stats()["qkv0_table_bytes"] == table_bytes(on)
    on.close(), off.close()


def test_row_1_of_two_rows_is_the_one_row_run(golden):
    """What the dot-product table rests on: the kernel's row result at M = 2 (row 1) and at M = 1 is the same function of the id.  On
    the engine without the table every layer's in-projection -- layer 0's too -- runs at M = 2 and at M = 1; the table engine agrees."""
    g = golden("decoder_S")
    on, off = pair(g, max_batch=8, max_ctx=256)
    p0, p1 = g["prompt0"].tolist(), g["prompt1"].tolist()
    two = off.generate([p0, p1], 120, top_k=1).cpu()
    one = off.generate([p1], 120, top_k=1).cpu()
    assert torch.equal(two[1], one[0])
    assert torch.equal(on.generate([p0, p1], 120, top_k=1).cpu(), two) and torch.equal(on.generate([p1], 120, top_k=1).cpu(), one)
    on.close(), off.close()


def test_an_engine_that_serves_both_paths_owns_both_tables(golden):
    g = golden("decoder_tiny8h")
    on = make(g, 1, max_batch=8)
    prompts = [g[f"prompt{i % 3}"].tolist() for i in range(8)]
    on.generate(prompts[:1], 8, top_k=1)
    assert on.stats()["qkv0_table_bytes"] == table_bytes(on)
    on.generate(prompts, 8, top_k=1)
    assert on.stats()["qkv0_table_bytes"] == 2 * table_bytes(on)
    on.close()
