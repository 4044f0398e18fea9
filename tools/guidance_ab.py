"""What classifier-free guidance costs per decode step ("Classifier-free guidance"; profiles/guidance_ab.txt).

Decoder-S (6L / 512d / V 8324), f32, 64 rows, top-k 50, one engine, one build:
  guided    32 pairs: 32 prompts of --prompt tokens with their 32 one-token negative prompts as shadow rows, scale 1.5 --
            generate_guided, the SAMPLED form's launch sequence with the mix launch between the head and the sampler;
  unguided  the same 64 prompts as 64 independent rows -- generate_rows, the SAMPLED form as it always was.
Both run the same GEMM / attention kernels on the same 64 rows and cached lengths; what differs is the one launch.  A step's time is a
difference of two generations, (t(n0 + steps) - t(n0)) / steps, so the prefill and the call's fixed costs cancel.  The two alternate
--reps times; the medians are reported, one JSON line.

    python tools/guidance_ab.py [--reps 5] [--steps 256]
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
from mgea.decoder import DecoderEngine, RowSampling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=6)
    args = ap.parse_args()
    V, L, C, NL, N0, PAIRS = 8324, 1024, 512, 6, 16, 32
    eng = DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=2 * PAIRS, max_ctx=L)
    rng = np.random.default_rng(5)
    prompts = [[int(v) for v in rng.integers(0, V, args.prompt)] for _ in range(PAIRS)]
    negs = [p[:1] for p in prompts]
    rows = [RowSampling(1.0, 50, seed=3) for _ in range(PAIRS)]

    def timed(guided, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if guided:
            eng.generate_guided(prompts, negs, rows, 1.5, n)
        else:
            eng.generate_rows(prompts + negs, rows + rows, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_us(guided):
        return 1e6 * (timed(guided, N0 + args.steps) - timed(guided, N0)) / args.steps

    for guided in (True, False):   # warm-up: every graph captured, the qkv0 table built
        step_us(guided)
    g, u = [], []
    for _ in range(args.reps):
        g.append(step_us(True))
        u.append(step_us(False))
    eng.generate_guided(prompts, negs, rows, 1.5, 1)
    nodes_g, info = eng.stats()["graph_nodes"], eng.guidance_info()
    eng.generate_rows(prompts + negs, rows + rows, 1)
    nodes_u = eng.stats()["graph_nodes"]
    mg, mu = statistics.median(g), statistics.median(u)
    print(json.dumps(dict(steps=args.steps, reps=args.reps, rows=2 * PAIRS, pairs=info["pairs"], top_k=50, scale=1.5,
                          graph_nodes=dict(guided=nodes_g, unguided=nodes_u),
                          us_per_step=dict(guided=round(mg, 2), unguided=round(mu, 2), difference=round(mg - mu, 2),
                                           guided_all=[round(v, 2) for v in g], unguided_all=[round(v, 2) for v in u]))), flush=True)


if __name__ == "__main__":
    main()
