"""What a KV window costs per decode step ("KV window"; profiles/window_step_ab.txt).

Decoder-S (6L / 512d / V 8324), f32, B = 64 and B = 1, greedy and top-k 50.  Three engines of max_ctx 1024 (16 pages a row, so the
attention takes one grid in all of them) in one process:
  windowed    set_window(1, 7): P = 8 pages.  A 40-token prompt fills them after i0 = 471 steps; the --steps steps after that all run
              at a full cache, 448 .. 511 cached tokens (mean 479.5), every one behind the evict launch and with page ids from the table.
  unwindowed  a prompt of 464 - steps / 2 tokens and 16 steps first, so that its --steps steps run at the same MEAN cached length
              (a ramp of steps tokens around 480 against the window's saw: an unwindowed row cannot stay at one length).
  table       unwindowed, its graphs captured with the switch attn_arith_pages = 0: page ids from the table in the attention and the
              step's tail, as under a window, without the evict launch -- the control that separates the window's two costs.
A step's time is a difference of two generations, (t(n0 + steps) - t(n0)) / steps, so the prefill, the call's fixed costs and the
steps before cancel (n0 = i0 windowed, 16 otherwise).  The engines alternate --reps times; the medians are reported, one JSON line.

    python tools/window_step_bench.py [--reps 3] [--steps 256]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mgea import _lib, synth  # noqa: E402
from mgea.decoder import DecoderEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    args = ap.parse_args()
    V, L, C, NL, CTX, LP, RING, N0 = 8324, 1024, 512, 6, 1024, 40, 7, 16
    sd = synth.decoder_state_dict(21, V, L, C, NL)
    plain = DecoderEngine(sd, n_head=8, max_batch=64, max_ctx=CTX)
    win = DecoderEngine(sd, n_head=8, max_batch=64, max_ctx=CTX)
    table = DecoderEngine(sd, n_head=8, max_batch=64, max_ctx=CTX)
    win.set_window(1, RING, max_steps=2048)
    i0 = win.window.first_eviction_step(LP)
    rng = np.random.default_rng(5)
    short = [int(v) for v in rng.integers(0, V, LP)]
    long = [int(v) for v in rng.integers(0, V, 64 * (1 + RING) - 32 - N0 - args.steps // 2)]   # the same mean cached length

    def timed(eng, prompt, B, n, top_k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate([prompt] * B, n, top_k=top_k, seed=3)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_us(eng, prompt, B, n0, top_k):
        return 1e6 * (timed(eng, prompt, B, n0 + args.steps, top_k) - timed(eng, prompt, B, n0, top_k)) / args.steps

    cases = [(B, k) for B in (64, 1) for k in (1, 50)]
    for B, k in cases:   # warm-up: every graph captured, the qkv0 tables built
        step_us(win, short, B, i0, k)
        step_us(plain, long, B, N0, k)
        old = _lib.tune_set("attn_arith_pages", 0)   # read when a step is enqueued: the control's graphs are captured under it
        try:
            step_us(table, long, B, N0, k)
        finally:
            _lib.tune_set("attn_arith_pages", old)
    res = {}
    for B, k in cases:
        w, p, t = [], [], []
        for _ in range(args.reps):
            w.append(step_us(win, short, B, i0, k))
            p.append(step_us(plain, long, B, N0, k))
            t.append(step_us(table, long, B, N0, k))
        name = f"B{B}_{'greedy' if k == 1 else 'top_k50'}"
        res[name] = dict(windowed_us=round(statistics.median(w), 2), unwindowed_us=round(statistics.median(p), 2),
                         table_us=round(statistics.median(t), 2), windowed_all=[round(v, 2) for v in w],
                         unwindowed_all=[round(v, 2) for v in p], table_all=[round(v, 2) for v in t])
    win.generate([short], i0 + args.steps, top_k=1)
    print(json.dumps(dict(steps=args.steps, reps=args.reps, window=dict(sink_pages=1, ring_pages=RING), i0=i0,
                          evictions=win.window_evictions()[:1], graph_nodes=dict(windowed=win.stats()["graph_nodes"],
                                                                                 unwindowed=plain.stats()["graph_nodes"]),
                          us_per_step=res)), flush=True)


if __name__ == "__main__":
    main()
