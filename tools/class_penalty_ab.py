"""What a windowed class penalty costs per decode step ("Windowed penalties over token classes";
profiles/class_penalty_ab.txt).

Decoder-S (6L / 512d / V 8324), f32, 64 rows, top-k 50, one engine, one build, a KV window of 1 + 15 pages so that a generation can
run past 4096 steps: every row carries the same ClassPenalty(frequency 0.01, presence 0.5, window W) for W in --windows over a map of
128 classes (id % 128), against the same 64 prompts without a record -- the SAMPLED form as it always was.  A step's time is a
difference of two generations, (t(n0 + steps) - t(n0)) / steps with n0 = 4096, so the prefill and the call's fixed costs cancel and
every timed step counts a FULL window (t >= 4096 >= W).  The forms alternate --reps times; the medians are reported.  On a library
without the feature only the plain step is measured (null elsewhere), so the tool also runs on the parent commit.  One JSON line.

    python tools/class_penalty_ab.py [--reps 3] [--steps 256] [--windows 32,1024,4096]
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

from mgea import synth  # noqa: E402
from mgea import decoder as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--n0", type=int, default=4096)
    ap.add_argument("--prompt", type=int, default=6)
    ap.add_argument("--windows", default="32,1024,4096")
    args = ap.parse_args()
    windows = [int(w) for w in args.windows.split(",")]
    V, L, C, NL, ROWS = 8324, 1024, 512, 6, 64
    rng = np.random.default_rng(5)
    eng = D.DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=ROWS, max_ctx=L)
    eng.set_window(1, None, max_steps=args.n0 + args.steps)
    can = hasattr(eng, "set_penalty_classes")
    if can:
        eng.set_penalty_classes(np.arange(V) % 128)
    prompts = [[int(v) for v in rng.integers(0, V, args.prompt)] for _ in range(ROWS)]

    def rows(W):
        if not W:
            return [D.RowSampling(1.0, 50, seed=3)] * ROWS
        return [D.RowSampling(1.0, 50, seed=3, class_penalty=D.ClassPenalty(0.01, 0.5, W))] * ROWS

    def timed(W, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate_rows(prompts, rows(W), n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_us(W):
        return 1e6 * (timed(W, args.n0 + args.steps) - timed(W, args.n0)) / args.steps

    forms = [0] + (windows if can else [])   # 0 = no record
    for W in forms:   # warm-up: every graph captured, the qkv0 table built
        step_us(W)
    runs = {W: [] for W in forms}
    for _ in range(args.reps):
        for W in forms:
            runs[W].append(step_us(W))
    med = {W: statistics.median(v) for W, v in runs.items()}
    nodes, info = {}, None
    for W in forms:
        timed(W, 1)
        nodes["plain" if W == 0 else str(W)] = eng.stats()["graph_nodes"]
        if W:
            info = eng.class_penalty_info()
    print(json.dumps(dict(steps=args.steps, n0=args.n0, reps=args.reps, rows=ROWS, top_k=50, n_class=128,
                          graph_nodes=nodes, last_class_penalty_info=info,
                          us_per_step=dict(plain=round(med[0], 2),
                                           penalized={str(W): (round(med[W], 2) if W in med else None) for W in windows},
                                           difference={str(W): (round(med[W] - med[0], 2) if W in med else None) for W in windows},
                                           all={("plain" if W == 0 else str(W)): [round(v, 2) for v in vs] for W, vs in runs.items()}))),
          flush=True)


if __name__ == "__main__":
    main()
