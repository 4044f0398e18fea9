#!/usr/bin/env python3
"""Decoder-S prefill [64, 1024] (non-causal, no past, logits dropped like the sampler): time, tokens/s and TFLOP/s vs the MFMA
peak of the dtype (3.86 TFLOP incl. the head; without head 3.30).   python3 tools/prefill_bench.py [f32|f16] [logits]
--causal (instead): the same prefill on a reference-mode and a pos_mode="causal" engine built from the same weights, in one process,
alternating (ROUNDS alternations after warm-up; the causal engine with both walks of the dense attention's grid, switch attn_causal_walk): the median and the spread of the single runs of each.   python3 tools/prefill_bench.py [f32|f16] --causal"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))
import torch
from mgea import synth
from mgea.decoder import DecoderEngine
B, T = 64, 1024
DEC = dict(vocab=8324, seq_len=1024, d_model=512, n_layer=6, d_ff=2048)
sd = synth.decoder_state_dict(0, DEC["vocab"], DEC["seq_len"], DEC["d_model"], DEC["n_layer"])
args = [a for a in sys.argv[1:] if not a.startswith("--")]
dtype = args[0] if args else "f32"
peak = 157.3 if dtype == "f32" else 2500.0
eng = DecoderEngine(sd, n_head=8, max_batch=B, max_ctx=T, dtype=dtype)
ids = torch.from_numpy(synth.integers(1, "p", (B, T), 0, DEC["vocab"])).cuda()
if "--causal" in sys.argv[1:]:
    import statistics
    from mgea import _lib
    ROUNDS = 9
    ceng = DecoderEngine(sd, n_head=8, max_batch=B, max_ctx=T, dtype=dtype, pos_mode="causal")
    def run(e, walk):
        _lib.tune_set("attn_causal_walk", walk)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e.reset_and_prefill(ids, want_logits=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    forms = (("reference", eng, 1), ("causal pairs-first", ceng, 1), ("causal block-order", ceng, 2))
    ms = {k: [] for k, _, _ in forms}
    for r in range(ROUNDS + 2):
        for k, e, walk in forms:
            t = run(e, walk)
            if r >= 2: ms[k].append(t)   # two warm-up rounds
    _lib.tune_set("attn_causal_walk", 1)
    for k, _, _ in forms:
        v = sorted(ms[k])
        print(f"prefill [64,1024] {dtype} {k:16s}: median {statistics.median(v):.2f} ms  min {v[0]:.2f}  max {v[-1]:.2f}  ({len(v)} runs, alternating)")
    sys.exit(0)
for want_logits in ((False, True) if "logits" in args[1:] else (False,)):
    for _ in range(2): eng.reset_and_prefill(ids, want_logits=want_logits)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n = 3
    for _ in range(n): eng.reset_and_prefill(ids, want_logits=want_logits)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    C, NL, V = 512, 6, 8324
    flops = 2 * B * T * (NL * 12 * C * C) + 4 * B * T * T * C * NL + (2 * B * T * V * C if want_logits else 0)
    print(f"prefill [64,1024] {dtype} logits={want_logits}: {dt*1e3:.2f} ms  {B*T/dt:.0f} tok/s  {flops/dt/1e12:.1f} TFLOP/s ({flops/dt/1e12/peak:.3f} of the {dtype} MFMA peak)")
