"""Per-launch time of the sampler under a token grammar ("Token grammars"; profiles/grammar_step_ab.txt).

Decoder-S (6L / 512d / V 8324), f32, B = 64 and B = 1, 256 decode steps from the endpoint's prompt, top-p 0.92 with penalty 1.1
and the notes-only bias of generate_music.constraints on every row.  Every --stride-th step of a generation runs eagerly with HIP
events around each launch (DecoderEngine.profile); the `sample` class of that profile is one sampler launch per step.  Forms:
"biased" (the BIASED step form) and "grammar" (the same rows with the track grammar of the vocabulary, start state OPEN: the
GRAMMAR form).  Prints one JSON line per repeat, the forms interleaved inside a repeat.  A checkout from before the grammar skips
that form, so the same script measures the parent commit.

    python tools/grammar_step_bench.py [--reps 3] [--stride 8] [--steps 256]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))

import torch  # noqa: E402

from generate_music import constraints  # noqa: E402
from mgea import synth  # noqa: E402
from mgea.decoder import DecoderEngine, RowSampling  # noqa: E402

PROMPT = ["[START_SEQUENCE]", "[BPM] 120", "[KEY_SIGNATURE] C major", "[INSTRUMENT] Violin", "[INSTRUMENT] Flute"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    args = ap.parse_args()
    V, L, C, NL = 8324, 1024, 512, 6
    eng = DecoderEngine(synth.decoder_state_dict(21, V, L, C, NL), n_head=8, max_batch=64, max_ctx=L)
    tok2id = synth.decoder_vocab(V, with_eos=True)
    prompt = [tok2id[t] for t in PROMPT]
    bias = torch.from_numpy(constraints.logit_bias(tok2id)).to(eng.device)
    forms = ["biased"]
    start = None
    if hasattr(eng, "set_grammar"):
        from generate_music.grammar import start_state, track_grammar
        gram = track_grammar(tok2id)
        eng.set_grammar(gram)
        start = start_state(gram, prompt)
        forms.append("grammar")

    def run(form, B):
        extra = dict(grammar_state=start) if form == "grammar" else {}
        rows = [RowSampling(1.0, 0, 0.92, 1.1, seed=1 + b, logit_bias=bias, **extra) for b in range(B)]
        return eng.generate_rows([prompt] * B, rows, args.steps)

    for B in (64, 1):
        for f in forms:   # warm-up: every graph captured
            run(f, B)
    torch.cuda.synchronize()
    for rep in range(args.reps):
        res = {}
        for B in (64, 1):
            for f in forms:
                eng.profile(args.stride)
                run(f, B)
                eng.profile(0)
                r = eng.profile_read()["sample"]
                res[f"{f}_B{B}"] = round(1000.0 * r["ms"] / max(r["launches"], 1), 3)
        print(json.dumps(dict(rep=rep, steps=args.steps, us_per_sampler_launch=res)), flush=True)


if __name__ == "__main__":
    main()
