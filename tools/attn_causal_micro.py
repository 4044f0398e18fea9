"""Dense f32 attention alone at the Decoder-S prefill shape [64, 1024, 8 x 64]: the non-causal kernel against the causal one in both
grid walks (switch attn_causal_walk), HIP events, 10 alternations after 2 warm-ups (profiles/causal_prefill_ab.txt, section 3).
  python3 tools/attn_causal_micro.py"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))
import torch
from mgea import ops, _lib
B, T, H, dh = 64, 1024, 8, 64
g = torch.Generator().manual_seed(1)
qkv = ((torch.rand(B, T, 3 * H * dh, generator=g) * 2 - 1) * 1.5).cuda()
out = torch.empty(B, T, H * dh, device="cuda")
forms = [("non-causal", False, 1), ("causal pairs-first", True, 1), ("causal block-order", True, 2)]
ms = {k: [] for k, _, _ in forms}
for r in range(12):
    for k, c, w in forms:
        _lib.tune_set("attn_causal_walk", w)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.attention(qkv, H, out=out, causal=c); e1.record(); torch.cuda.synchronize()
        if r >= 2: ms[k].append(e0.elapsed_time(e1) * 1e3)
for k, _, _ in forms:
    v = sorted(ms[k]); print(f"{k:20s}: median {statistics.median(v):8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}")
_lib.tune_set("attn_causal_walk", 1)
