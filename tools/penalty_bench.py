"""Cost of the repetition penalty per decode step of generate() ("Repetition penalty").

Decoder-S (6L / 512d / V 8324), f32, B = 1 and B = 64: greedy with and without p = 1.1, top-k 50 with and without p = 1.1,
and the paper's top-p 0.92 + p = 1.1.  Each A/B pair is timed alternately in the same process (device events around whole
generate() calls, after a warm-up that captures every graph), so drift hits both sides alike.  Prints one JSON line per
(batch, setting): the median microseconds per decode step over --reps alternations.

    python tools/penalty_bench.py [--steps 256] [--reps 7]
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
from mgea.decoder import DecoderEngine  # noqa: E402

SETTINGS = {   # name -> generate() keywords
    "greedy": dict(top_k=1),
    "greedy+p1.1": dict(top_k=1, repetition_penalty=1.1),
    "topk50": dict(top_k=50, seed=1),
    "topk50+p1.1": dict(top_k=50, seed=1, repetition_penalty=1.1),
    "topp0.92+p1.1": dict(top_k=0, top_p=0.92, seed=1, repetition_penalty=1.1),
}
PAIRS = [("greedy", "greedy+p1.1"), ("topk50", "topk50+p1.1"), ("topp0.92+p1.1",)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,64")
    a = ap.parse_args()
    V, L, C, NL = 8324, 1024, 512, 6
    sd = synth.decoder_state_dict(21, V, L, C, NL)
    eng = DecoderEngine(sd, n_head=8, max_batch=64, max_ctx=L)
    rng = np.random.default_rng(0)
    for B in (int(b) for b in a.batches.split(",")):
        prompts = [list(rng.integers(0, V, 16)) for _ in range(B)]

        def timed(kw):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            eng.generate(prompts, a.steps, 1.0, **kw)
            ev1.record()
            torch.cuda.synchronize()
            return ev0.elapsed_time(ev1) * 1e3 / a.steps   # us per step (prefill included, amortised)

        for kw in SETTINGS.values():   # warm-up: every graph captured
            timed(kw)
            timed(kw)
        res = {k: [] for k in SETTINGS}
        for _ in range(a.reps):
            for pair in PAIRS:
                for name in pair:
                    res[name].append(timed(SETTINGS[name]))
        for name, v in res.items():
            print(json.dumps(dict(batch=B, setting=name, us_per_step=round(statistics.median(v), 2),
                                  spread=round(max(v) - min(v), 2), steps=a.steps, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
