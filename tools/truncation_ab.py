"""What min-p, typical-p, the epsilon and the eta cutoff cost in the HIP sampler ("Truncation").

Decoder-S (6L / 512d / V 8324), f32, B = 64, 5-token prompts, penalty 1.1 on every form.
  * per sampler launch: every --stride-th step of a 1019-step generate_rows() runs eagerly with HIP events around each launch
    (DecoderEngine.profile); the sampler class of that profile is one launch_sample per step.  Forms: the biased form with top-p 0.92
    (a dense finite bias; the path a request took before there were truncation records), then top_k = 0 with each stage alone and
    with all four.
  * per decode step: (t(16 + --steps steps) - t(16 steps)) / --steps of whole generations, the biased top-p 0.92 form against
    typical_p 0.9, alternated.
Prints one JSON line per repeat, the forms interleaved inside a repeat.  Forms the library does not have (a checkout from before the
truncation records) are skipped, so the same script measures the parent commit.

    python tools/truncation_ab.py [--reps 3] [--stride 8] [--steps 256]
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

import mgea.decoder as dec  # noqa: E402
from mgea import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    args = ap.parse_args()
    V, L, C, NL, B = 8324, 1024, 512, 6, 64
    eng = dec.DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=B, max_ctx=L)
    rng = np.random.default_rng(5)
    prompts = [list(rng.integers(0, V, 5)) for _ in range(B)]
    bias = torch.from_numpy((rng.standard_normal(V) * 2).astype(np.float32)).cuda()
    forms = [("biased_topp092", dict(top_k=0, top_p=0.92, logit_bias=bias))]
    if hasattr(dec, "Truncation"):
        T = dec.Truncation
        forms += [("min_p_005", dict(top_k=0, truncation=T(min_p=0.05))), ("typical_p_09", dict(top_k=0, truncation=T(typical_p=0.9))),
                  ("typical_p_02", dict(top_k=0, truncation=T(typical_p=0.2))), ("epsilon_3e-4", dict(top_k=0, truncation=T(epsilon_cutoff=3e-4))),
                  ("eta_2e-3", dict(top_k=0, truncation=T(eta_cutoff=2e-3))),
                  ("all_four", dict(top_k=0, truncation=T(0.02, 0.8, 1e-4, 1e-3))),
                  ("topp092_all_four", dict(top_k=0, top_p=0.92, truncation=T(0.02, 0.8, 1e-4, 1e-3)))]

    def run(kw, n):
        rows = [dec.RowSampling(temperature=1.0, repetition_penalty=1.1, seed=1, **kw) for _ in range(B)]
        return eng.generate_rows(prompts, rows, n, check_bias=False)

    for _, kw in forms:   # warm-up: every graph captured
        run(kw, L - 5)
        run(kw, 16)
    torch.cuda.synchronize()

    def timed(kw, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(kw, n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    step_forms = [f for f in forms if f[0] in ("biased_topp092", "typical_p_09")]
    for rep in range(args.reps):
        res = {}
        for name, kw in forms:
            eng.profile(args.stride)
            run(kw, L - 5)
            eng.profile(0)
            r = eng.profile_read()["sample"]
            res[name] = round(1000.0 * r["ms"] / max(r["launches"], 1), 3)
        step = {}
        for name, kw in step_forms:
            step[name] = round(1e6 * (timed(kw, 16 + args.steps) - timed(kw, 16)) / args.steps, 2)
        print(json.dumps(dict(rep=rep, us_per_sampler_launch=res, us_per_decode_step=step)), flush=True)


if __name__ == "__main__":
    main()
