"""mgea.serve.RequestBatcher on a stub engine (no GPU): coalescing of queued requests into one generation, the max_batch cap,
per-request settings and budgets, reproducible seeds, errors in the caller's thread and in one batch only, and close()."""
import threading

import pytest
import torch

from test_row_sampler_host import StubEngine, stub_model


class GatedEngine(StubEngine):
    """generate_rows waits for `gate` (when set) and raises for a prompt that contains `poison`."""

    def __init__(self, *a, poison=None, **kw):
        super().__init__(*a, **kw)
        self.gate, self.poison, self.entered = None, poison, threading.Event()

    def generate_rows(self, prompts, rows, n_steps=None):
        self.entered.set()
        if self.gate is not None:
            assert self.gate.wait(10)
        if self.poison is not None and any(self.poison in p for p in prompts):
            raise RuntimeError("engine failure")
        return super().generate_rows(prompts, rows, n_steps)


def test_queued_requests_run_as_one_generation():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    b = RequestBatcher(m, autostart=False)
    futs = [b.submit(names[3 + i:5 + 2 * i], max_len=10 + i, top_k=1, seed=i) for i in range(6)]
    b.start()
    outs = [f.result(timeout=10) for f in futs]
    b.close()
    assert b.stats() == dict(generations=1, rows_per_generation=[6], requests=6)
    assert len(m.engine.calls) == 1 and len(m.engine.calls[0]["prompts"]) == 6
    for i, (f, o) in enumerate(zip(futs, outs)):
        assert o[:len(names[3 + i:5 + 2 * i])] == names[3 + i:5 + 2 * i] and len(o) == 10 + i
        assert f.batch_rows == 6


def test_batches_are_capped_at_max_batch():
    from mgea.serve import RequestBatcher
    m, gen = stub_model(max_batch=8)
    names = list(gen.tok2id)
    b = RequestBatcher(m, max_batch=4, autostart=False)
    assert RequestBatcher(m, autostart=False).max_batch == 8   # default: the engine's
    futs = [b.submit(names[1:3], max_len=8, seed=1) for _ in range(6)]
    b.start()
    for f in futs:
        f.result(timeout=10)
    b.close()
    assert b.stats()["rows_per_generation"] == [4, 2]
    assert [f.batch_rows for f in futs] == [4] * 4 + [2] * 2


def test_idle_worker_starts_at_once_and_later_requests_queue():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    m.engine = GatedEngine(64)
    names = list(gen.tok2id)
    m.engine.gate = threading.Event()
    b = RequestBatcher(m)
    first = b.submit(names[1:3], max_len=8, seed=1)
    assert m.engine.entered.wait(10)          # started alone, with no waiting window
    rest = [b.submit(names[4:6], max_len=9, seed=2) for _ in range(3)]
    m.engine.gate.set()
    for f in [first] + rest:
        f.result(timeout=10)
    b.close()
    assert b.stats()["rows_per_generation"] == [1, 3]


def test_settings_and_budgets_reach_the_engine():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    b = RequestBatcher(m, autostart=False)
    b.submit(names[1:4], max_len=20, temperature=0.7, top_k=1, seed=11)
    b.submit(names[5:7], max_len=12, top_k=50, top_p=0.92, repetition_penalty=1.1, seed=12)
    b.submit(names[8:9], max_len=30, temperature=1.3, top_k=0, seed=13)
    b.start()
    b.close()
    call, = m.engine.calls
    rows = call["rows"]
    assert [r.max_new_tokens for r in rows] == [17, 10, 29] and call["n_steps"] == 29
    assert [(r.temperature, r.top_k, r.top_p, r.repetition_penalty, r.seed) for r in rows] == \
        [(0.7, 1, None, None, 11), (1.0, 50, 0.92, 1.1, 12), (1.3, 0, None, None, 13)]
    assert all(r.stream == 0 and r.eos_id == gen.tok2id["[END_SEQUENCE]"] for r in rows)


def test_torch_manual_seed_makes_drawn_seeds_reproducible():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    seeds = []
    for _ in range(2):
        b = RequestBatcher(m, autostart=False)
        torch.manual_seed(123)
        for i in range(3):
            b.submit(names[1 + i:3 + i], max_len=8)
        b.start()
        b.close()
        seeds.append([r.seed for r in m.engine.calls[-1]["rows"]])
    assert seeds[0] == seeds[1] and len(set(seeds[0])) == 3


def test_unknown_token_raises_at_submit():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    b = RequestBatcher(m)
    with pytest.raises(KeyError):
        b.submit(["[START_SEQUENCE]", "no such token"], max_len=8)
    with pytest.raises(ValueError):
        b.submit(["[START_SEQUENCE]"], max_len=8, repetition_penalty=0.0)
    b.close()
    assert b.stats()["generations"] == 0 and not m.engine.calls


def test_engine_error_fails_only_its_batch():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    m.engine = GatedEngine(64, poison=gen.tok2id[names[7]])
    b = RequestBatcher(m, max_batch=2, autostart=False)
    bad = [b.submit(names[6:8], max_len=8, seed=1), b.submit(names[1:3], max_len=8, seed=2)]
    good = [b.submit(names[1:3], max_len=8, seed=3)]
    b.start()
    for f in bad:
        with pytest.raises(RuntimeError, match="engine failure"):
            f.result(timeout=10)
    assert len(good[0].result(timeout=10)) == 8
    b.close()
    assert b.stats()["rows_per_generation"] == [2, 1]


def test_close():
    from mgea.serve import RequestBatcher
    m, gen = stub_model()
    names = list(gen.tok2id)
    b = RequestBatcher(m)
    f = b.submit(names[1:3], max_len=8, seed=1)
    b.close()
    assert f.done() and len(f.result()) == 8
    assert b._thread is not None and not b._thread.is_alive()
    with pytest.raises(RuntimeError):
        b.submit(names[1:3], max_len=8)
    with pytest.raises(RuntimeError):
        b.start()
    idle = RequestBatcher(m, autostart=False)     # never started: its queued requests fail
    g = idle.submit(names[1:3], max_len=8, seed=1)
    idle.close()
    with pytest.raises(RuntimeError, match="closed"):
        g.result(timeout=1)
