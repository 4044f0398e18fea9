"""Cost of the scored sampler ("Log-probabilities and forced ids").

Decoder-S (6L / 512d / V 8324), f32, B = 64.
  --mode gen   : wall time of a 1019-step generation from 5-token prompts, top-k 50, the SAMPLED form (generate_rows) against its
                 scored twin (generate_scored), interleaved, one JSON line per repeat;
  --mode op    : --iters launches each of the plain and the scored sampler over one [64, 8324] logits matrix (ops.sample_rows /
                 ops.sample_rows_scored), for `rocprofv3 --kernel-trace --stats -- python tools/logprobs_bench.py --mode op`:
                 the two kernels' rows of the statistics are the per-launch times.

    python tools/logprobs_bench.py [--mode gen] [--reps 3] [--iters 200]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mgea import ops, synth  # noqa: E402
from mgea.decoder import DecoderEngine, RowSampling  # noqa: E402

V, L, C, NL, B = 8324, 1024, 512, 6, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("gen", "op"), default="gen")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    rows = [RowSampling(1.0, 50, seed=1) for _ in range(B)]
    if args.mode == "op":
        logits = torch.from_numpy((rng.standard_normal((B, V)) * 3).astype(np.float32)).cuda()
        for i in range(args.iters):
            ops.sample_rows(logits, rows, step=i)
            ops.sample_rows_scored(logits, rows, step=i)
        torch.cuda.synchronize()
        print(json.dumps(dict(mode="op", launches_each=args.iters)))
        return
    eng = DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=B, max_ctx=L)
    prompts = [list(rng.integers(0, V, 5)) for _ in range(B)]
    forms = (("sampled", lambda: eng.generate_rows(prompts, rows, L - 5)), ("scored", lambda: eng.generate_scored(prompts, rows, L - 5)))
    for _, fn in forms:   # warm-up: every graph captured
        fn()
    torch.cuda.synchronize()
    for rep in range(args.reps):
        res = {}
        for name, fn in forms:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[name] = round(1000.0 * (time.perf_counter() - t0), 2)
        print(json.dumps(dict(rep=rep, steps=L - 5, ms_per_generation=res)), flush=True)


if __name__ == "__main__":
    main()
