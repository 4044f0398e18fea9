"""What tests/test_transitions_host.py and tests/test_gpu_transitions.py share: the oracle of a scheduled generation -- DecoderRef
with its per-layer (K, V) cache spliced at the steps the host model of the rule (mgea.decoder.RowSchedule.segment_at) names -- and
the one case both files use, so that the CPU file can assert the premise of the GPU file on the very same inputs.

The case: the golden tiny8h geometry (256 wide, 8 heads, 2 layers, vocabulary 300), rows of 1, 2 and 3 segments in one batch, 24
steps teacher-forced on the oracle's own greedy ids of the UNSWITCHED first variant.  The variants of the scheduled rows are random ids,
kept from a search over the ORACLE alone for prompts whose switch moves the forced id's log-probability at every later step by more
than 0.03 (tests/test_transitions_host.py asserts the premise; with variants that differ in two tokens only, as a [BPM] / [KEY_SIGNATURE]
swap does, the smallest per-step difference over 24 steps falls to 5e-4 on this geometry: a splice the tolerance could hide)."""
import functools
import os

import numpy as np
import torch

from mgea import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAG = "tiny8h"
N_STEPS = 24
# per row: its prompt variants and its thresholds (key 0: step indices).  Rows 0-2 are the 3-row batch; the 9-row batch is all of them.
ROWS = [
    ([[64, 79, 40, 275, 152], [83, 235, 287, 89, 269], [230, 238, 158, 273, 45]], (5, 13)),
    ([[1, 7, 20, 33, 34, 40, 3]], ()),
    ([[174, 35, 260, 170], [268, 217, 84, 206]], (8,)),
    ([[70, 227, 244, 34, 273, 3], [39, 62, 177, 151, 202, 255]], (0,)),
    ([[2, 9]], ()),
    ([[30, 78, 238, 232, 135], [154, 183, 260, 175, 151], [228, 116, 296, 193, 194]], (3, 4)),
    ([[147, 265, 56, 272], [221, 238, 94, 62]], (23,)),
    ([[1, 5, 11, 26, 27, 28, 29, 35]], ()),
    ([[151, 295, 92, 144, 246], [105, 262, 29, 69, 259]], (12,)),
]


@functools.lru_cache(maxsize=None)
def model(tag=TAG):
    seed, vocab, seq_len, d_model, n_head, n_layer = (int(x) for x in np.load(os.path.join(GOLDEN, f"decoder_{tag}.npz"))["cfg"])
    return synth.decoder_state_dict(seed, vocab, seq_len, d_model, n_layer), n_head, vocab


def rounded(sd):
    """the model an fp16 engine serves: the five matrix kinds rounded to fp16 (tests/test_gpu_f16.py)"""
    from mgea.decoder import F16_ROUNDED_KEYS
    return {k: (torch.from_numpy(np.asarray(v)).float().half().float() if k.endswith(F16_ROUNDED_KEYS) else torch.from_numpy(np.asarray(v)).float())
            for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def oracle(tag=TAG, f16=False):
    from oracle.decoder_ref import DecoderRef
    sd, n_head, _ = model(tag)
    return DecoderRef(rounded(sd) if f16 else sd, n_head)


def oracle_scheduled(ref, variants, schedule, n_steps, forced=None, grammar=None, start_state=None, splice=True):
    """One row of a scheduled generation on the oracle: prefill every variant alone, start from variant 0's cache, and at the start
    of every step put the K | V of positions [0, len) of the segment the host model names over the cache's -- every layer --
    whenever it differs from the row's current segment.  The key is the step index, or with a grammar the row's state (the start
    state, then moved by every fed id).  forced None: greedy.  splice=False: the same loop without any switch (the premise's
    other side).  Returns (ids, float64 log-probability of every id, the segment of every step)."""
    n = len(variants[0])
    caches = [ref.forward(torch.tensor([v]))[1] for v in variants]
    cache = [(k.clone(), v.clone()) for k, v in caches[0]]
    last = torch.tensor([[variants[0][-1]]])
    cur, state = 0, start_state
    ids, lps, segs = [], [], []
    for i in range(n_steps):
        seg = schedule.segment_at(state if schedule.key else i)
        if splice and seg != cur:
            for (k, v), (ks, vs) in zip(cache, caches[seg]):
                k[:, :n] = ks[:, :n]
                v[:, :n] = vs[:, :n]
            cur = seg
        segs.append(cur)
        logits, cache, _ = ref.forward(last, cache)
        cache = [(k.clone(), v.clone()) for k, v in cache]
        lg = logits[0, -1]
        t = int(lg.argmax()) if forced is None else int(forced[i])
        ids.append(t)
        lps.append(float(torch.log_softmax(lg.double(), dim=0)[t]))
        if grammar is not None:
            state = grammar.step(state, t)
        last = torch.tensor([[t]])
    return ids, torch.tensor(lps, dtype=torch.float64), segs


def schedules():
    from mgea.decoder import RowSchedule
    return [RowSchedule(tuple(th), 0) for _, th in ROWS]


@functools.lru_cache(maxsize=None)
def reference(f16=False):
    """The case's oracle runs, once: per row (forced ids, spliced log-probabilities, unspliced log-probabilities, segments).  The
    forced ids are the f32 oracle's greedy ids of the unswitched first variant."""
    out = []
    for (variants, _), sc in zip(ROWS, schedules()):
        forced, _, _ = oracle_scheduled(oracle(), variants, sc, N_STEPS, splice=False)
        _, want, segs = oracle_scheduled(oracle(f16=f16), variants, sc, N_STEPS, forced)
        _, plain, _ = oracle_scheduled(oracle(f16=f16), variants, sc, N_STEPS, forced, splice=False)
        out.append((forced, want, plain, segs))
    return out
