"""What a prompt schedule costs per decode step ("Emotion transitions"; profiles/recondition_ab.txt).

Decoder-S (6L / 512d / V 8324), f32, 64 rows, top-k 50, one engine, one build, every row with two prompt variants of --prompt tokens:
  never        generate_scheduled with a threshold beyond the call: every step opens with the apply launch, no row ever switches --
               the launch's loads and its branch, 256 times;
  switch       generate_scheduled in which all 64 rows switch at the same step, in the middle of the measured steps: the same plus
               ONE step that copies 64 rows x 6 layers of prompt K | V (switch_us: that step's extra time, the difference to `never`
               times the steps);
  unscheduled  the same first prompts through generate_rows, the SAMPLED form as it always was.
All run the same GEMM / attention kernels on the same 64 rows and cached lengths.  A step's time is a difference of two generations,
(t(n0 + steps) - t(n0)) / steps, so the prefills -- a scheduled call has one per variant -- the gathers and the call's fixed costs
cancel; the short run ends before the switch.  The three alternate --reps times; the medians are reported, one JSON line.

    python tools/recondition_ab.py [--reps 5] [--steps 256]
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
from mgea.decoder import DecoderEngine, RowSampling, RowSchedule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=6)
    args = ap.parse_args()
    V, L, C, NL, N0, B = 8324, 1024, 512, 6, 16, 64
    eng = DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=B, max_ctx=L)
    rng = np.random.default_rng(5)
    first = [[int(v) for v in rng.integers(0, V, args.prompt)] for _ in range(B)]
    segs = [[p, p[:1] + [int(v) for v in rng.integers(0, V, args.prompt - 2)] + p[-1:]] for p in first]
    rows = [RowSampling(1.0, 50, seed=3) for _ in range(B)]
    at = N0 + args.steps // 2
    kinds = dict(never=[RowSchedule((10 ** 9,))] * B, switch=[RowSchedule((at,))] * B, unscheduled=None)

    def timed(kind, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kinds[kind] is None:
            eng.generate_rows(first, rows, n)
        else:
            eng.generate_scheduled(segs, rows, kinds[kind], n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def step_us(kind):
        return 1e6 * (timed(kind, N0 + args.steps) - timed(kind, N0)) / args.steps

    for kind in kinds:   # warm-up: every graph captured, the qkv0 table built, the store allocated
        step_us(kind)
    got = {kind: [] for kind in kinds}
    switches = {}
    for _ in range(args.reps):
        for kind in kinds:
            got[kind].append(step_us(kind))
            switches[kind] = eng.schedule_info()["switches"]   # of the short run: 0 everywhere
    nodes = {}
    for kind in kinds:
        timed(kind, 1)
        nodes[kind] = eng.stats()["graph_nodes"]
    timed("switch", N0 + args.steps)
    switched = eng.schedule_info()["switches"]
    med = {kind: statistics.median(v) for kind, v in got.items()}
    print(json.dumps(dict(steps=args.steps, reps=args.reps, rows=B, prompt_tokens=args.prompt, top_k=50, switch_at_step=at,
                          switches=dict(never=switches["never"], switch=switched), graph_nodes=nodes,
                          us_per_step=dict({k: round(v, 2) for k, v in med.items()},
                                           never_minus_unscheduled=round(med["never"] - med["unscheduled"], 2),
                                           switch_us=round((med["switch"] - med["never"]) * args.steps, 1),
                                           **{k + "_all": [round(x, 2) for x in v] for k, v in got.items()}))), flush=True)


if __name__ == "__main__":
    main()
