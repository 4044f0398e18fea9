"""Cost of per-row sampler records per decode step ("Per-row sampling").

Decoder-S (6L / 512d / V 8324), f32, B = 64: a sampled step (top-k 50) and a penalized step (top-p 0.92 + p 1.1), each with uniform
records (generate()) and with mixed records (generate_rows: per row another temperature, top-k / top-p, seed and stream; the
penalized pair also mixes p = 1 rows in).  Pairs are timed alternately in one process (device events around whole calls, after a
warm-up that captures every graph).  Prints one JSON line per setting: the median microseconds per decode step over --reps.

    python tools/row_sampler_bench.py [--steps 256] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mgea import synth  # noqa: E402
from mgea.decoder import DecoderEngine, RowSampling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    V, L, C, NL = 8324, 1024, 512, 6
    B = a.batch
    eng = DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=B, max_ctx=L)
    rng = np.random.default_rng(0)
    prompts = [list(rng.integers(0, V, 16)) for _ in range(B)]
    mixed_topk = [RowSampling(temperature=0.7 + 0.01 * b, top_k=(50, 1, 20, 0)[b % 4], top_p=(None, None, 0.9, 0.95)[b % 4],
                              seed=b + 1, stream=0) for b in range(B)]
    mixed_pen = [RowSampling(temperature=1.0, top_k=(0, 50, 1, 0)[b % 4], top_p=0.92, repetition_penalty=(1.1, 1.0, 1.2, 1.05)[b % 4],
                             seed=b + 1, stream=0) for b in range(B)]
    settings = {
        "topk50 uniform": lambda: eng.generate(prompts, a.steps, 1.0, top_k=50, seed=1),
        "topk50 mixed": lambda: eng.generate_rows(prompts, mixed_topk, a.steps),
        "topp0.92+p1.1 uniform": lambda: eng.generate(prompts, a.steps, 1.0, top_k=0, top_p=0.92, seed=1, repetition_penalty=1.1),
        "topp0.92+p1.1 mixed": lambda: eng.generate_rows(prompts, mixed_pen, a.steps),
    }

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / a.steps   # us per step (prefill included, amortised)

    for fn in settings.values():   # warm-up: every graph captured
        timed(fn)
        timed(fn)
    res = {k: [] for k in settings}
    for _ in range(a.reps):
        for name, fn in settings.items():
            res[name].append(timed(fn))
    for name, v in res.items():
        print(json.dumps(dict(batch=B, setting=name, us_per_step=round(statistics.median(v), 2), spread=round(max(v) - min(v), 2),
                              steps=a.steps, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
