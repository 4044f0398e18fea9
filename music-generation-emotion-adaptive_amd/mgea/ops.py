"""Thin torch-tensor wrappers over the op-level C entry points (mgea_op_* in include/mgea.h).
Used by the parity tests to check single kernels; the engines do not go through these."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import SamplerConfig, check, ptr, stream_ptr


def _dev(t: torch.Tensor) -> torch.Tensor:
    if t.device.type != "cuda":
        raise RuntimeError("mgea ops need ROCm device tensors; there is no CPU path")
    return t.contiguous()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, split_k: int = 0) -> torch.Tensor:
    """a [M,K] @ w[N,K]^T (+ bias): exact-fp32 MFMA GEMM with deterministic split-K."""
    lib = _lib.load()
    a, w = _dev(a.float()), _dev(w.float())
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({M}x{K} and {w.shape[1]}x{N})")
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    slabs = split_k if split_k > 0 else (32 if M <= 64 else 1)
    ws = torch.empty(max(1, lib.mgea_op_gemm_workspace_floats(M, N, slabs)), dtype=torch.float32, device=a.device)
    b = None if bias is None else _dev(bias.float())
    check(lib.mgea_op_gemm_f32(ptr(a), ptr(w), ptr(b), ptr(out), M, N, K, split_k, ptr(ws), stream_ptr()))
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    lib = _lib.load()
    x, w, b = _dev(x.float()), _dev(w.float()), _dev(b.float())
    M, Cd = x.shape
    y = torch.empty_like(x)
    check(lib.mgea_op_layernorm(ptr(x), ptr(w), ptr(b), ptr(y), M, Cd, float(eps), stream_ptr()))
    return y


def attention(qkv: torch.Tensor, n_head: int, lens: Optional[torch.Tensor] = None,
              mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv [B,T,3C] -> [B,T,C]; non-causal, keys valid per lens / mask."""
    lib = _lib.load()
    qkv = _dev(qkv.float())
    B, T, C3 = qkv.shape
    Cd = C3 // 3
    out = torch.empty(B, T, Cd, dtype=torch.float32, device=qkv.device)
    l32 = None if lens is None else _dev(lens.to(torch.int32))
    m32 = None if mask is None else _dev(mask.to(torch.int32))
    check(lib.mgea_op_attention_f32(ptr(qkv), ptr(l32), ptr(m32), ptr(out), B, T, n_head, Cd // n_head, stream_ptr()))
    return out


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
              gelu: bool = False, ln: Optional[dict] = None, info: Optional[list] = None, out: Optional[torch.Tensor] = None):
    """bf16 perf-mode GEMM: (a [M,K] bf16) @ (w [N,K] bf16)^T + bias (fp32) [+GELU | +res (bf16)] -> bf16.
    ln (persistent 256 x 256 kernel only) selects a LayerNorm-folding epilogue of the big-batch DistilBERT pipeline (mgea.h):
      dict(rowstat=[M,2], c1=[N])                      -> epi 3 / 4 (gelu): rstd (a w'^T - mean c1) + bias, bias = c2
      dict(rowstat=[M,2], g=[N], b=[N], stats=True)    -> epi 5: a w^T + bias + LN(res); returns (out, per-tile (sum, M2) [M, N/256, 2])
    info: a list that receives [kernel, half_tiles] of the launch."""
    lib = _lib.load()
    a, w = _dev(a.to(torch.bfloat16)), _dev(w.to(torch.bfloat16))
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    b = None if bias is None else _dev(bias.float())
    r = None if res is None else _dev(res.to(torch.bfloat16))
    epi = 2 if res is not None else (1 if gelu else 0)
    rowstat = c1 = g = be = stats = None
    if ln is not None:
        rowstat = _dev(ln["rowstat"].float())
        if "c1" in ln:
            epi, c1 = (4 if gelu else 3), _dev(ln["c1"].float())
        else:
            epi, g, be = 5, _dev(ln["g"].float()), _dev(ln["b"].float())
            if isinstance(ln.get("stats"), torch.Tensor):
                stats = ln["stats"]                                   # caller's [M, N/256, 2] fp32 buffer (benchmarks: no allocation per call)
            elif ln.get("stats"):
                stats = torch.zeros(M, N // 256, 2, dtype=torch.float32, device=a.device)
    io = (C.c_int32 * 2)(-1, -1)
    check(lib.mgea_op_gemm_bf16_ln(ptr(a), ptr(w), ptr(b), ptr(r), ptr(out), M, N, K, epi, ptr(rowstat), ptr(c1), ptr(g), ptr(be),
                                   ptr(stats), io, stream_ptr()))
    if info is not None:
        info[:] = [int(io[0]), int(io[1])]
    return (out, stats) if stats is not None else out


def ln_rowstat(part: torch.Tensor, C_: int, eps: float) -> torch.Tensor:
    """per-tile (sum, M2) [M, n_part, 2] -> (mean, rstd) [M, 2] of rows of C_ columns."""
    lib = _lib.load()
    part = _dev(part.float())
    M, n_part = part.shape[0], part.shape[1]
    out = torch.empty(M, 2, dtype=torch.float32, device=part.device)
    check(lib.mgea_op_ln_rowstat(ptr(part), ptr(out), M, n_part, int(C_), float(eps), stream_ptr()))
    return out


def fold_ln_bf16(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: torch.Tensor):
    """-> (bf16(W diag(gamma)) [N,K], c1 [N] = row sums of the rounded product, c2 [N] = bias + W beta)."""
    lib = _lib.load()
    w, gamma, beta, bias = _dev(w.float()), _dev(gamma.float()), _dev(beta.float()), _dev(bias.float())
    N, K = w.shape
    wf = torch.empty(N, K, dtype=torch.bfloat16, device=w.device)
    c1 = torch.empty(N, dtype=torch.float32, device=w.device)
    c2 = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib.mgea_op_fold_ln_bf16(ptr(w), ptr(gamma), ptr(beta), ptr(bias), N, K, ptr(wf), ptr(c1), ptr(c2), stream_ptr()))
    return wf, c1, c2


def attention_bf16(qkv: torch.Tensor, n_head: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    qkv = _dev(qkv.to(torch.bfloat16))
    B, T, C3 = qkv.shape
    Cd = C3 // 3
    out = torch.empty(B, T, Cd, dtype=torch.bfloat16, device=qkv.device)
    m32 = None if mask is None else _dev(mask.to(torch.int32))
    check(lib.mgea_op_attention_bf16(ptr(qkv), ptr(m32), ptr(out), B, T, n_head, Cd // n_head, stream_ptr()))
    return out


def layernorm_bf16(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    lib = _lib.load()
    x = _dev(x.to(torch.bfloat16))
    y = torch.empty_like(x)
    check(lib.mgea_op_layernorm_bf16(ptr(x), ptr(_dev(w.float())), ptr(_dev(b.float())), ptr(y), x.shape[0], x.shape[1],
                                     float(eps), stream_ptr()))
    return y


def check_repetition_penalty(penalty) -> Optional[float]:
    """None -> None (no penalty).  Otherwise the penalty as a float, which must be finite and > 0 also once held as
    fp32 (the kernels' precision): ValueError otherwise, as transformers' RepetitionPenaltyLogitsProcessor raises."""
    if penalty is None:
        return None
    p = float(penalty)
    with np.errstate(over="ignore"):
        p32 = float(np.float32(p))
    if not (math.isfinite(p32) and p32 > 0):
        raise ValueError(f"`repetition_penalty` has to be a finite, strictly positive float, but is {penalty}")
    return p


def presence_words(vocab: int) -> int:
    return (int(vocab) + 31) // 32


def pack_presence(presence, B: int, V: int) -> np.ndarray:
    """The presence bitmaps of the penalized sampler, uint32 [B, ceil(V / 32)]: bit id & 31 of word id >> 5 of row b is set iff
    id is seen in row b.  presence: a bool [B, V] mask (tensor or array), or B sequences of ids (repeats allowed)."""
    W = presence_words(V)
    if isinstance(presence, (torch.Tensor, np.ndarray)):
        m = presence.detach().cpu().numpy() if isinstance(presence, torch.Tensor) else np.asarray(presence)
        if m.shape != (B, V):
            raise ValueError(f"presence mask must be [{B}, {V}], got {list(m.shape)}")
        m = np.concatenate([m.astype(bool), np.zeros((B, W * 32 - V), bool)], axis=1).reshape(B, W, 32)
        return (m.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    rows = list(presence)
    if len(rows) != B:
        raise ValueError(f"presence needs {B} id lists, got {len(rows)}")
    out = np.zeros((B, W), np.uint32)
    for b, ids in enumerate(rows):
        ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= V):
            raise ValueError("presence ids must lie in [0, vocab)")
        np.bitwise_or.at(out[b], ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return out


def unpack_presence(words: torch.Tensor, V: int) -> torch.Tensor:
    """int32 / uint32 words [B, ceil(V / 32)] -> bool mask [B, V] (on the words' device)"""
    w = words.view(torch.int32) if words.dtype != torch.int32 else words
    bits = (w.unsqueeze(-1) >> torch.arange(32, dtype=torch.int32, device=w.device)) & 1
    return bits.reshape(w.shape[0], -1)[:, :V].bool()


def sample(logits: torch.Tensor, temperature=1.0, top_k=50, top_p=None, seed=0, step=0, want_probs=False,
           repetition_penalty=None, presence=None):
    """repetition_penalty (None = none): the logits of the ids in `presence` (a bool [B, V] mask or B id lists; none if
    None) are penalized first, x < 0 ? x * p : x / p, as in mgea_decoder_generate_penalized; top_k=1 then takes the argmax of
    the penalized row."""
    pen = check_repetition_penalty(repetition_penalty)
    lib = _lib.load()
    logits = _dev(logits.float())
    B, V = logits.shape
    s = SamplerConfig(temperature=float(temperature), top_k=int(top_k) if top_k else 0,
                      top_p=float(top_p) if top_p else 0.0, eos_id=-1, seed=int(seed))
    ids = torch.empty(B, dtype=torch.int32, device=logits.device)
    probs = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_probs else None
    if pen is None:
        check(lib.mgea_op_sample(ptr(logits), B, V, C.byref(s), int(step), ptr(ids), ptr(probs), stream_ptr()))
    else:
        words = pack_presence(presence if presence is not None else [[] for _ in range(B)], B, V)
        bits = torch.from_numpy(words.view(np.int32)).to(logits.device)
        check(lib.mgea_op_sample_penalized(ptr(logits), B, V, C.byref(s), pen, ptr(bits), int(step), ptr(ids), ptr(probs),
                                           stream_ptr()))
    return (ids, probs) if want_probs else ids


def sample_biased(logits: torch.Tensor, temperature=1.0, top_k=50, top_p=None, seed=0, step=0, want_probs=False,
                  repetition_penalty=None, presence=None, logit_bias=None):
    """sample() with a logit bias (sample()'s own parameter list is kept as it is).  logit_bias: None (then this IS sample()), one
    vector for all rows -- a dict id -> bias, a host array or a device tensor [V] -- or [B, V]: added to the penalized logits, -inf
    bans an id.  With a bias this is sample_rows() with the same record on every row: the same draws."""
    if logit_bias is None:
        return sample(logits, temperature, top_k, top_p, seed, step, want_probs, repetition_penalty, presence)
    from .decoder import RowSampling
    row = RowSampling(temperature, top_k, top_p, check_repetition_penalty(repetition_penalty), -1, 0, seed)
    return sample_rows(logits, [row] * logits.shape[0], step, want_probs, presence, logit_bias=logit_bias)


def sample_rows(logits: torch.Tensor, rows, step=0, want_probs=False, presence=None, logit_bias=None, min_new_tokens=None):
    """sample() with one mgea.decoder.RowSampling per row (mgea_op_sample_rows): row b reads rows[b] and draws from Philox counter
    (stream_b, step) under key seed_b (stream None = b).  presence (a bool [B, V] mask or B id lists) is what the penalized rows
    penalize; none if None.  top_k=1 rows take the exact argmax of their (penalized) row, without the temperature division.
    logit_bias (one vector for all rows or [B, V]) and min_new_tokens (an int or one per row) override the rows' own fields; a row
    with either goes through mgea_op_sample_rows_biased: bias added after the penalty, eos_id banned while step < min_new_tokens."""
    return _sample_rows(logits, rows, step, want_probs, presence, logit_bias, min_new_tokens, False, None)


def sample_rows_scored(logits: torch.Tensor, rows, step=0, want_probs=False, presence=None, logit_bias=None, min_new_tokens=None,
                       forced=None):
    """sample_rows() through the scored sampler (mgea_op_sample_rows_scored): returns (ids, logprobs, choice_logprobs[, probs]) --
    logprobs [B] = log-softmax of the RAW logits row at the id, choice_logprobs [B] = the id's log-probability under the
    distribution in probs (-inf outside the kept set).  forced: None, or B ints (a list or an int tensor), -1 = draw; a row with a
    forced id >= 0 takes it instead of its draw."""
    return _sample_rows(logits, rows, step, want_probs, presence, logit_bias, min_new_tokens, True, forced)


def _sample_rows(logits: torch.Tensor, rows, step, want_probs, presence, logit_bias, min_new_tokens, scored, forced):
    """sample_rows / sample_rows_scored: pack the rows, one native call."""
    import dataclasses
    from .decoder import pack_row_logits, pack_rows
    rows = list(rows)
    if logit_bias is not None or min_new_tokens is not None:
        nb = len(rows)
        per_row = [logit_bias] * nb
        if logit_bias is not None and not isinstance(logit_bias, dict) and getattr(logit_bias, "ndim", 1) == 2:
            if logit_bias.shape[0] != nb:
                raise ValueError(f"logit_bias must be [V] or [{nb}, V], got {list(logit_bias.shape)}")
            per_row = [logit_bias[b] for b in range(nb)]
        mins = list(min_new_tokens) if isinstance(min_new_tokens, (list, tuple)) else [min_new_tokens] * nb
        rows = [dataclasses.replace(r, logit_bias=r.logit_bias if logit_bias is None else per_row[b],
                                    min_new_tokens=r.min_new_tokens if mins[b] is None else int(mins[b]))
                for b, r in enumerate(rows)]
    lib = _lib.load()
    logits = _dev(logits.float())
    B, V = logits.shape
    recs = pack_rows(rows, V)
    if len(recs) != B:
        raise ValueError(f"{B} logits rows but {len(recs)} sampler rows")
    bits = None
    if any(r.repetition_penalty != 1.0 for r in recs):
        words = pack_presence(presence if presence is not None else [[] for _ in range(B)], B, V)
        bits = torch.from_numpy(words.view(np.int32)).to(logits.device)
    ids = torch.empty(B, dtype=torch.int32, device=logits.device)
    probs = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_probs else None
    lrecs, keep = pack_row_logits(rows, V, logits.device)
    if scored:
        f = None
        if forced is not None:
            f = torch.as_tensor(forced).to(device=logits.device, dtype=torch.int32).contiguous()
            if f.shape != (B,):
                raise ValueError(f"forced must hold {B} ids, got {list(f.shape)}")
        lp = torch.empty(B, dtype=torch.float32, device=logits.device)
        ch = torch.empty(B, dtype=torch.float32, device=logits.device)
        check(lib.mgea_op_sample_rows_scored(ptr(logits), B, V, recs, ptr(bits), lrecs, int(step), ptr(ids), ptr(probs), ptr(f), ptr(lp),
                                             ptr(ch), stream_ptr()))
        return (ids, lp, ch, probs) if want_probs else (ids, lp, ch)
    if lrecs is None:
        check(lib.mgea_op_sample_rows(ptr(logits), B, V, recs, ptr(bits), int(step), ptr(ids), ptr(probs), stream_ptr()))
    else:
        check(lib.mgea_op_sample_rows_biased(ptr(logits), B, V, recs, ptr(bits), lrecs, int(step), ptr(ids), ptr(probs), stream_ptr()))
    return (ids, probs) if want_probs else ids


def tile_weights(w: torch.Tensor) -> torch.Tensor:
    """W [N,K] row-major -> the fragment-ordered layout the skinny GEMM reads (rows padded to 32)."""
    lib = _lib.load()
    w = _dev(w.float())
    N, K = w.shape
    out = torch.empty(lib.mgea_op_tiled_weight_floats(N, K), dtype=torch.float32, device=w.device)
    check(lib.mgea_op_tile_weights(ptr(w), N, K, ptr(out), stream_ptr()))
    return out


def tile_rows(x: torch.Tensor) -> torch.Tensor:
    """[M<=512, N] row-major -> k-tiled activation buffer (whole 64-row groups of 64 * N floats; rows >= M are zero)."""
    lib = _lib.load()
    x = _dev(x.float())
    M, N = x.shape
    out = torch.zeros((M + 63) // 64 * 64 * N, dtype=torch.float32, device=x.device)
    check(lib.mgea_op_tile_rows(ptr(x), ptr(out), M, N, 1, stream_ptr()))
    return out


def untile_rows(t: torch.Tensor, M: int, N: int) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty(M, N, dtype=torch.float32, device=t.device)
    check(lib.mgea_op_tile_rows(ptr(_dev(t)), ptr(out), M, N, 0, stream_ptr()))
    return out


def fold_ln(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: torch.Tensor):
    """LayerNorm folded into the matrix it feeds -> (tiled gamma * W, c1, c2); see mgea_op_fold_ln."""
    lib = _lib.load()
    w, gamma, beta, bias = _dev(w.float()), _dev(gamma.float()), _dev(beta.float()), _dev(bias.float())
    N, K = w.shape
    wt = torch.empty(lib.mgea_op_tiled_weight_floats(N, K), dtype=torch.float32, device=w.device)
    c1 = torch.empty(N, dtype=torch.float32, device=w.device)
    c2 = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib.mgea_op_fold_ln(ptr(w), ptr(gamma), ptr(beta), ptr(bias), N, K, ptr(wt), ptr(c1), ptr(c2), stream_ptr()))
    return wt, c1, c2


def skinny(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, *, residual: Optional[torch.Tensor] = None,
           act: int = 0, ln: Optional[tuple] = None, dbg: int = 0):
    """The fused decode-step GEMM on row-major inputs (tiling / folding done here): epilogue `residual` (returns
    (residual + a @ w^T + bias, per-16-column (mean, M2) statistics)) or activation `act` (0 none, 1 GELU,
    2 ReLU).  ln = (gamma, beta, stats [M, K/16, 2]) applies LayerNorm to `a` from 16-column partial statistics."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    at = tile_rows(a)
    c1 = st = None
    n_part = 0
    if ln is not None:
        wt, c1, b = fold_ln(w, ln[0], ln[1], bias)
        st = _dev(ln[2].float())
        n_part = st.shape[1]
    else:
        wt, b = tile_weights(w), _dev(bias.float())
    stats_out = torch.zeros(max(64, M) * (N // 16) * 2 + 4096, dtype=torch.float32, device=a.device)
    if residual is not None:
        out = tile_rows(residual)
        check(lib.mgea_op_skinny(1, ptr(at), ptr(wt), ptr(b), ptr(c1), ptr(st), n_part, 16, ptr(out), ptr(stats_out),
                                 M, N, K, 0, dbg, stream_ptr()))
        return untile_rows(out, M, N), stats_out[:M * (N // 16) * 2].view(M, N // 16, 2)
    out = torch.zeros((M + 63) // 64 * 64 * N, dtype=torch.float32, device=a.device)
    check(lib.mgea_op_skinny(2, ptr(at), ptr(wt), ptr(b), ptr(c1), ptr(st), n_part, 16, ptr(out), ptr(stats_out),
                             M, N, K, act, dbg, stream_ptr()))
    return untile_rows(out, M, N)


def head(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, want_logits: bool = True):
    """The LM head of a decode step (api_cache.py:105) on row-major inputs: returns (logits [M, N] or None, argmax [M] int64 merged from
    the per-workgroup (max, argmax) partials the kernel leaves for the greedy tail, partial count P).  Which kernel runs -- the balanced
    one-round kernel of csrc/head_gemm.hip or the generic skinny kernel -- follows the library's own routing (switch head_balanced)."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    at, wt, b = tile_rows(a), tile_weights(w), _dev(bias.float())
    P = int(lib.mgea_op_skinny_logits_partials(M, N, K))
    R = max(64, M)   # rows of each half of the partials buffer (mgea.h)
    part = torch.full((2 * R * P + 64,), float("nan"), dtype=torch.float32, device=a.device)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=a.device) if want_logits else None
    check(lib.mgea_op_skinny(3, ptr(at), ptr(wt), ptr(b), None, None, 0, 16, ptr(out), ptr(part), M, N, K, 0, 0, stream_ptr()))
    val = part[: R * P].view(R, P)[:M]
    idx = part[R * P: 2 * R * P].view(torch.int32).view(R, P)[:M].long()
    best = val.max(1, keepdim=True).values
    cand = torch.where(val == best, idx, torch.full_like(idx, 2 ** 31 - 1))
    return out, cand.min(1).values, P
