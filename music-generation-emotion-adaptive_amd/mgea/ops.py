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
              mask: Optional[torch.Tensor] = None, cu: Optional[torch.Tensor] = None, tiled: bool = False,
              out: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """qkv [B,T,3C] -> [B,T,C]; non-causal, keys valid per lens / mask.  causal: query i sees the keys t <= i that lens leaves valid
    (mgea_op_attention_f32_causal; mask and cu are the launcher's refusal, RuntimeError).  cu [B + 1] (packed rows): qkv [cu[B], 3C] -> [cu[B], C], T = the
    longest sequence.  tiled: the output is the flat k-tiled buffer of tiled_floats(B * T, C) floats (untile_rows reads it).  out: a
    caller buffer of that many floats (B * T * C row-major), written in place and returned.  What the launcher refuses (cu with lens,
    mask or tiled) is left to the launcher."""
    lib = _lib.load()
    qkv = _dev(qkv.float())
    Cd = qkv.shape[-1] // 3
    c32 = None
    if cu is not None:
        c32 = _dev(cu.to(torch.int32))
        seq = (cu[1:] - cu[:-1]).cpu()
        B, T = int(seq.numel()), int(seq.max())
        if qkv.ndim != 2 or int(cu[-1]) != qkv.shape[0]:
            raise RuntimeError("packed attention: qkv must be [cu[B], 3C]")
        rows = qkv.shape[0]
    else:
        B, T = qkv.shape[0], qkv.shape[1]
        rows = B * T
    if out is None:
        out = (torch.empty(tiled_floats(rows, Cd), dtype=torch.float32, device=qkv.device) if tiled
               else torch.empty(*qkv.shape[:-1], Cd, dtype=torch.float32, device=qkv.device))
    else:
        _buf(out, tiled_floats(rows, Cd) if tiled else rows * Cd, torch.float32, "attention: out")
    l32 = None if lens is None else _dev(lens.to(torch.int32))
    m32 = None if mask is None else _dev(mask.to(torch.int32))
    if causal:
        if mask is not None or cu is not None:   # what launch_attn_dense answers to causal with a mask or packed rows
            raise RuntimeError("attention: the causal form takes no mask and no packed rows")
        check(lib.mgea_op_attention_f32_causal(ptr(qkv), ptr(l32), ptr(out), B, T, n_head, Cd // n_head, int(bool(tiled)), stream_ptr()))
        return out
    check(lib.mgea_op_attention_f32_ex(ptr(qkv), ptr(l32), ptr(m32), ptr(c32), ptr(out), B, T, n_head, Cd // n_head, int(bool(tiled)),
                                       stream_ptr()))
    return out


attention_f32 = attention   # (the C entry point's name)


def logprob_gather(logits: torch.Tensor, targets, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = logits[m, targets[m]] - logsumexp(logits[m]) (mgea_op_logprob_gather): logits [M, V] fp32 on the device, rows of any
    stride; targets [M] ints, < 0 = not scored (0).  A target >= V in HOST targets (a list or a CPU tensor) is a RuntimeError, the
    library's MGEA_EINVAL; device targets are not read back and clamp to V - 1.  out: a caller buffer of at least M floats."""
    if logits.device.type != "cuda" or logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("logprob_gather: logits must be a [M, V] fp32 device tensor with unit column stride")
    M, V = logits.shape
    t = targets if isinstance(targets, torch.Tensor) else torch.tensor(list(targets), dtype=torch.int32)
    if t.numel() != M:
        raise RuntimeError(f"logprob_gather: {M} rows but {t.numel()} targets")
    if t.device.type != "cuda" and M and int(t.max()) >= V:
        raise RuntimeError(f"logprob_gather: target {int(t.max())} outside the vocabulary of {V}")
    t32 = t.to(device=logits.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=logits.device)
    else:
        _buf(out, M, torch.float32, "logprob_gather: out")
    check(_lib.load().mgea_op_logprob_gather(ptr(logits), logits.stride(0), ptr(t32), ptr(out), M, V, stream_ptr()))
    return out


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
              gelu: bool = False, ln: Optional[dict] = None, info: Optional[list] = None, out: Optional[torch.Tensor] = None,
              epi: Optional[int] = None):
    """bf16 perf-mode GEMM: (a [M,K] bf16) @ (w [N,K] bf16)^T + bias (fp32) [+GELU | +res (bf16)] -> bf16.
    ln (persistent 256 x 256 kernel only) selects a LayerNorm-folding epilogue of the big-batch DistilBERT pipeline (mgea.h):
      dict(rowstat=[M,2], c1=[N])                      -> epi 3 / 4 (gelu): rstd (a w'^T - mean c1) + bias, bias = c2
      dict(rowstat=[M,2], g=[N], b=[N], stats=True)    -> epi 5: a w^T + bias + LN(res); returns (out, per-tile (sum, M2) [M, N/256, 2])
    info: a list that receives [kernel, half_tiles] of the launch.  epi overrides the choice, and an ln entry may be None (the
    launcher's refusals)."""
    lib = _lib.load()
    a, w = _dev(a.to(torch.bfloat16)), _dev(w.to(torch.bfloat16))
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    b = None if bias is None else _dev(bias.float())
    r = None if res is None else _dev(res.to(torch.bfloat16))
    e = 2 if res is not None else (1 if gelu else 0)
    rowstat = c1 = g = be = stats = None
    opt = lambda t: None if t is None else _dev(t.float())
    if ln is not None:
        rowstat = opt(ln["rowstat"])
        if "c1" in ln:
            e, c1 = (4 if gelu else 3), opt(ln["c1"])
        else:
            e, g, be = 5, opt(ln["g"]), opt(ln["b"])
            if isinstance(ln.get("stats"), torch.Tensor):
                stats = ln["stats"]                                   # caller's [M, N/256, 2] fp32 buffer (benchmarks: no allocation per call)
            elif ln.get("stats"):
                stats = torch.zeros(M, N // 256, 2, dtype=torch.float32, device=a.device)
    if epi is not None:
        e = int(epi)
    io = (C.c_int32 * 2)(-1, -1)
    check(lib.mgea_op_gemm_bf16_ln(ptr(a), ptr(w), ptr(b), ptr(r), ptr(out), M, N, K, e, ptr(rowstat), ptr(c1), ptr(g), ptr(be),
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


# ---- the 16-bit kernels of the fp16 decoder and the paged attention (mgea_op_* of the same names) ----
_DTYPE16 = {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def _dtype16(t: torch.Tensor) -> int:
    if t.dtype not in _DTYPE16:
        raise RuntimeError(f"a bf16 or fp16 tensor is needed, got {t.dtype}")
    return _DTYPE16[t.dtype]


def gemm_f16_ln(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                gelu: bool = False, ln: Optional[dict] = None, f32_out: bool = False, info: Optional[list] = None,
                epi: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """gemm_bf16's folded-LayerNorm epilogues on fp16 operands (persistent kernel only): ln as in gemm_bf16 -> epi 3 / 4 (gelu) / 5,
    fp16 output; f32_out -> epi 6, a w^T + bias as fp32 [M, N].  epi overrides the choice (the launcher's refusals)."""
    lib = _lib.load()
    a, w = _dev(a.half()), _dev(w.half())
    M, K = a.shape
    N = w.shape[0]
    b = None if bias is None else _dev(bias.float())
    r = None if res is None else _dev(res.half())
    rowstat = c1 = g = be = stats = None
    e = 6 if f32_out else -1
    if ln is not None:
        rowstat = None if ln.get("rowstat") is None else _dev(ln["rowstat"].float())
        if "c1" in ln:
            e, c1 = (4 if gelu else 3), (None if ln["c1"] is None else _dev(ln["c1"].float()))
        else:
            e, g, be = 5, _dev(ln["g"].float()), _dev(ln["b"].float())
            if ln.get("stats"):
                stats = torch.zeros(M, N // 256, 2, dtype=torch.float32, device=a.device)
    if epi is not None:
        e = int(epi)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if e == 6 else torch.float16, device=a.device)
    io = (C.c_int32 * 2)(-1, -1)
    check(lib.mgea_op_gemm_f16_ln(ptr(a), ptr(w), ptr(b), ptr(r), ptr(out), M, N, K, e, ptr(rowstat), ptr(c1), ptr(g), ptr(be),
                                  ptr(stats), io, stream_ptr()))
    if info is not None:
        info[:] = [int(io[0]), int(io[1])]
    return (out, stats) if stats is not None else out


def gemm16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
           gelu: bool = False, ln: Optional[dict] = None, f32_out: bool = False, reverse: bool = False,
           info: Optional[list] = None, epi: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """gemm_bf16 / gemm_f16_ln as the engines launch them (mgea_op_gemm16): the type is a's (bf16 or fp16), and the leading
    dimensions are the tensors' row strides, so a [M, K], w [N, K], res and out [M, N] may be column or row slices of wider buffers.
    Nothing is copied: every operand must already be a device tensor of the right type with inner stride 1, res with the row stride
    of out (the kernels have one ldc for both).  ln, gelu, f32_out, epi as in gemm_f16_ln (ln["stats"] may be the caller's buffer);
    reverse asks for the persistent kernel's reversed tile walk.  info receives [kernel, half_tiles, tail_mode]."""
    lib = _lib.load()
    f16 = _dtype16(a) == _lib.DTYPE_F16
    if w.dtype != a.dtype or a.ndim != 2 or w.ndim != 2 or w.shape[1] != a.shape[1]:
        raise RuntimeError(f"gemm16: a {tuple(a.shape)} {a.dtype} and w {tuple(w.shape)} {w.dtype} do not multiply")
    M, K = a.shape
    N = w.shape[0]
    rowstat = c1 = g = be = stats = None
    e = 6 if f32_out else 2 if res is not None else 1 if gelu else 0
    if ln is not None:
        rowstat = ln.get("rowstat")
        if "c1" in ln:
            e, c1 = (4 if gelu else 3), ln["c1"]
        else:
            e, g, be = 5, ln["g"], ln["b"]
            if isinstance(ln.get("stats"), torch.Tensor):
                stats = ln["stats"]
            elif ln.get("stats"):
                stats = torch.zeros(M, N // 256, 2, dtype=torch.float32, device=a.device)
    if epi is not None:
        e = int(epi)
    out_dtype = torch.float32 if e == 6 else a.dtype
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    if out.dtype != out_dtype or tuple(out.shape) != (M, N):
        raise RuntimeError(f"gemm16: out {tuple(out.shape)} {out.dtype}, [{M}, {N}] {out_dtype} expected")
    mats = [("a", a), ("w", w), ("out", out)]
    if res is not None:
        if res.dtype != a.dtype or tuple(res.shape) != (M, N) or res.stride(0) != out.stride(0):
            raise RuntimeError("gemm16: res must have the type of a and the shape and row stride of out")
        mats.append(("res", res))
    for name, t in mats:
        if t.device.type != "cuda" or t.stride(1) != 1 or t.data_ptr() % 16:
            raise RuntimeError(f"gemm16: {name} must be a device tensor with inner stride 1 on a 16-byte boundary")
    for name, t in (("bias", bias), ("rowstat", rowstat), ("c1", c1), ("g", g), ("b", be), ("stats", stats)):
        if t is not None and not (t.device.type == "cuda" and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
            raise RuntimeError(f"gemm16: {name} must be a contiguous fp32 device tensor on a 16-byte boundary")
    io = (C.c_int32 * 3)(-1, -1, -1)
    check(lib.mgea_op_gemm16(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(res), ptr(out), out.stride(0), M, N, K, e,
                             int(f16), int(bool(reverse)), ptr(rowstat), ptr(c1), ptr(g), ptr(be), ptr(stats), io, stream_ptr()))
    if info is not None:
        info[:] = [int(io[0]), int(io[1]), int(io[2])]
    return (out, stats) if stats is not None else out


def f32_to_16(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 -> bf16 / fp16 by the library's convert kernel (round to nearest even)."""
    lib = _lib.load()
    x = _dev(x.float())
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib.mgea_op_f32_to_16(ptr(x), ptr(out), x.numel(), _dtype16(out), stream_ptr()))
    return out


def fold_ln_16(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: torch.Tensor, dtype: torch.dtype):
    """fold_ln_bf16 with the 16-bit type as an argument -> (dtype(W diag(gamma)) [N,K], c1, c2)."""
    lib = _lib.load()
    w, gamma, beta, bias = _dev(w.float()), _dev(gamma.float()), _dev(beta.float()), _dev(bias.float())
    N, K = w.shape
    wf = torch.empty(N, K, dtype=dtype, device=w.device)
    c1 = torch.empty(N, dtype=torch.float32, device=w.device)
    c2 = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib.mgea_op_fold_ln_16(ptr(w), ptr(gamma), ptr(beta), ptr(bias), N, K, _dtype16(wf), ptr(wf), ptr(c1), ptr(c2), stream_ptr()))
    return wf, c1, c2


def kv_page_elems(n_pages: int, n_head: int, head_dim: int) -> int:
    """elements of one layer of n_pages KV pages (csrc/common.h KvPool)"""
    return int(n_pages) * 2 * int(n_head) * _lib.KV_PAGE_TOKENS * int(head_dim)


def _int_view(t: torch.Tensor) -> torch.Tensor:
    """the same bits as integers (copies of these are bit copies whatever the floats are)"""
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def kv_pages_write(image: torch.Tensor, k: torch.Tensor, v: torch.Tensor, page_table, pos0=None, valid=None) -> torch.Tensor:
    """Host side of the page layout.  image: a CPU tensor of kv_page_elems(n_pages, H, dh) fp16 or fp32 elements (one layer of pages);
    k, v [B, T, H, dh] of the same dtype.  Token (b, t) with valid[b, t] (None: all) goes to position pos0[b] + t (None: t) of row b:
    logical page pos // 64 -> physical page_table[b][page], slot pos % 64; positions in logical pages >= page_table.shape[1] are
    dropped, as the kernels drop them.  K is [dh / G][64][G], V is [64][dh] per (page, K | V, head), G = 16 bytes of elements.
    Written in place, bit for bit; returns image."""
    B, T, H, dh = k.shape
    G = 16 // image.element_size()
    P = _lib.KV_PAGE_TOKENS
    table = np.asarray(page_table, dtype=np.int64).reshape(B, -1)
    n_pages = image.numel() // (2 * H * P * dh)
    img = _int_view(image).view(n_pages, 2, H, P * dh)
    ki, vi = _int_view(k.contiguous()), _int_view(v.contiguous())
    for b in range(B):
        t = np.arange(T) if valid is None else np.nonzero(np.asarray(valid[b]).astype(bool))[0]
        pos = t + (0 if pos0 is None else int(pos0[b]))
        keep = (pos // P) < table.shape[1]
        t, pos = t[keep], pos[keep]
        if t.size == 0:
            continue
        phys = torch.from_numpy(table[b][pos // P])
        slot = torch.from_numpy(pos % P)
        tt = torch.from_numpy(t)
        for h in range(H):
            kimg = img[:, 0, h].view(n_pages, dh // G, P, G)
            vimg = img[:, 1, h].view(n_pages, P, dh)
            kimg[phys, :, slot, :] = ki[b, tt, h].view(-1, dh // G, G)
            vimg[phys, slot, :] = vi[b, tt, h]
    return image


def kv_pages_read(image: torch.Tensor, page_table, b: int, n_tok: int, n_head: int, head_dim: int):
    """The first n_tok cached tokens of row b out of a page image (CPU tensor) -> (k, v) [n_tok, H, dh] in the image's dtype."""
    H, dh, P = n_head, head_dim, _lib.KV_PAGE_TOKENS
    G = 16 // image.element_size()
    table = np.asarray(page_table, dtype=np.int64).reshape(-1, np.asarray(page_table).shape[-1])
    n_pages = image.numel() // (2 * H * P * dh)
    img = image.view(n_pages, 2, H, P * dh)
    pos = np.arange(n_tok)
    phys, slot = torch.from_numpy(table[b][pos // P]), torch.from_numpy(pos % P)
    k = torch.stack([img[:, 0, h].view(n_pages, dh // G, P, G)[phys, :, slot, :].reshape(n_tok, dh) for h in range(H)], 1)
    v = torch.stack([img[:, 1, h].view(n_pages, P, dh)[phys, slot, :] for h in range(H)], 1)
    return k, v


def attention16(qkv: torch.Tensor, n_head: int, mask: Optional[torch.Tensor] = None, cu: Optional[torch.Tensor] = None,
                pages: Optional[torch.Tensor] = None, page_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 16-bit flash attention on a bf16 or fp16 qkv (its dtype picks the instantiation): [B, T, 3C] -> [B, T, C], or with cu
    [B + 1] (packed rows) [cu[B], 3C] -> [cu[B], C].  pages (fp16 only): one layer of device KV pages, written in place at position
    t for every key whose mask bit is set; page_table [B, max_pages] int32."""
    lib = _lib.load()
    if qkv.dtype not in _DTYPE16:
        raise RuntimeError("attention16 takes a bf16 or fp16 qkv")
    qkv = _dev(qkv)
    Cd = qkv.shape[-1] // 3
    dh = Cd // n_head
    m32 = None if mask is None else _dev(mask.to(torch.int32))
    c32 = None
    if cu is not None:
        c32 = _dev(cu.to(torch.int32))
        lens = (cu[1:] - cu[:-1]).cpu()
        B, T = int(lens.numel()), int(lens.max())
        if qkv.ndim != 2 or int(cu[-1]) != qkv.shape[0]:
            raise RuntimeError("packed attention16: qkv must be [cu[B], 3C]")
    else:
        B, T = qkv.shape[0], qkv.shape[1]
    out = torch.empty(*qkv.shape[:-1], Cd, dtype=qkv.dtype, device=qkv.device)
    n_pages = max_pages = 0
    pt = None
    if pages is not None:
        if pages.dtype != torch.float16 or pages.device != qkv.device or not pages.is_contiguous():
            raise RuntimeError("attention16: pages must be a contiguous fp16 device tensor")
        n_pages = pages.numel() // kv_page_elems(1, n_head, dh)
        pt = _dev(page_table.to(torch.int32))
        max_pages = pt.shape[1]
        if pt.shape[0] != B or int(pt.min()) < 0 or int(pt.max()) >= n_pages:
            raise RuntimeError("attention16: page table must be [B, max_pages] with entries in [0, n_pages)")
    check(lib.mgea_op_attention16(ptr(qkv), ptr(m32), ptr(c32), ptr(out), B, T, n_head, dh, _dtype16(qkv), ptr(pages), n_pages, ptr(pt),
                                  max_pages, stream_ptr()))
    return out


def kv_scatter_f16(qkv: torch.Tensor, n_head: int, pages: torch.Tensor, page_table: torch.Tensor, ctx_len: torch.Tensor,
                   lens: Optional[torch.Tensor] = None) -> None:
    """K | V of the fp16 qkv rows [B, T, 3C] into the fp16 device pages (in place) at positions ctx_len[b] + t, t < lens[b]."""
    lib = _lib.load()
    if qkv.dtype != torch.float16 or pages.dtype != torch.float16 or not pages.is_contiguous():
        raise RuntimeError("kv_scatter_f16 takes fp16 qkv rows and contiguous fp16 pages")
    qkv = _dev(qkv)
    B, T, C3 = qkv.shape
    dh = C3 // 3 // n_head
    n_pages = pages.numel() // kv_page_elems(1, n_head, dh)
    pt = _dev(page_table.to(torch.int32))
    if pt.shape[0] != B or int(pt.min()) < 0 or int(pt.max()) >= n_pages:
        raise RuntimeError("kv_scatter_f16: page table must be [B, max_pages] with entries in [0, n_pages)")
    cl = _dev(ctx_len.to(torch.int32))
    l32 = None if lens is None else _dev(lens.to(torch.int32))
    check(lib.mgea_op_kv_scatter_f16(ptr(qkv), ptr(pages), n_pages, ptr(pt), pt.shape[1], ptr(cl), ptr(l32), B, T, n_head, dh, stream_ptr()))


def dec_embed_f16(ids: torch.Tensor, tok_emb: torch.Tensor, pos_emb: torch.Tensor, lens: Optional[torch.Tensor] = None,
                  ctx_len: Optional[torch.Tensor] = None, absolute_pos: bool = False, eps: float = 1e-5):
    """The embedding kernel of the fp16 prefill on ids [B, T] -> (x [B, T, C] fp16, rowstat [B, T, 2], mask [B, T] int32, flags int)."""
    lib = _lib.load()
    ids = _dev(ids.to(torch.int32))
    tok_emb, pos_emb = _dev(tok_emb.float()), _dev(pos_emb.float())
    B, T = ids.shape
    V, Cd = tok_emb.shape
    dev = ids.device
    x = torch.empty(B, T, Cd, dtype=torch.float16, device=dev)
    rs = torch.empty(B, T, 2, dtype=torch.float32, device=dev)
    mk = torch.full((B, T), -1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    l32 = None if lens is None else _dev(lens.to(torch.int32))
    c32 = None if ctx_len is None else _dev(ctx_len.to(torch.int32))
    check(lib.mgea_op_dec_embed_f16(ptr(ids), ptr(l32), ptr(c32), ptr(tok_emb), ptr(pos_emb), ptr(x), ptr(rs), ptr(mk), float(eps), B, T, Cd,
                                    V, pos_emb.shape[0], int(bool(absolute_pos)), ptr(flag), stream_ptr()))
    return x, rs, mk, int(flag.item())


def attention_paged(qkv: torch.Tensor, n_head: int, pages: torch.Tensor, page_table: torch.Tensor, ctx_len: torch.Tensor,
                    lens: Optional[torch.Tensor] = None, arith_batch: int = 0, split: bool = True,
                    info: Optional[list] = None, layer: int = 0, n_layer: int = 1, tiled: bool = False,
                    out: Optional[torch.Tensor] = None, scratch=None, causal: bool = False) -> torch.Tensor:
    """The decode / extend attention over one layer of device KV pages (fp32 or fp16 tensor): the queries are columns 0..C-1 of the
    fp32 qkv [B, T, 3C]; row b attends to its ctx_len[b] + (lens[b] or T) cached tokens.  split=False: never the split-context form.
    info: a list that receives [workgroups per (row, head, query)] of the launch (1 = the unsplit kernel).
    pages holds n_layer layers of pages (one after the other, as in the decoder's pool) and the kernel reads `layer`.  tiled: the
    output is the flat k-tiled buffer of tiled_floats(B * T, C) floats.  out: a caller buffer of that size (B * T * C row-major),
    written in place and returned.  scratch = (part, count) from attn_split_scratch(): the caller's split-context scratch, which the
    call neither allocates nor zeroes.  causal: query (b, t) attends to its ctx_len[b] + t + 1 tokens, not to all the new ones
    (mgea_op_attention_paged_causal; T == 1 is the same launch either way)."""
    lib = _lib.load()
    qkv = _dev(qkv.float())
    B, T, C3 = qkv.shape
    Cd = C3 // 3
    dh = Cd // n_head
    if pages.dtype not in (torch.float32, torch.float16) or not pages.is_contiguous() or pages.device != qkv.device:
        raise RuntimeError("attention_paged: pages must be a contiguous fp32 or fp16 device tensor")
    n_pages = pages.numel() // (kv_page_elems(1, n_head, dh) * int(n_layer))
    pt = _dev(page_table.to(torch.int32))
    if pt.shape[0] != B or int(pt.min()) < 0 or int(pt.max()) >= n_pages:
        raise RuntimeError("attention_paged: page table must be [B, max_pages] with entries in [0, n_pages)")
    cl = _dev(ctx_len.to(torch.int32))
    l32 = None if lens is None else _dev(lens.to(torch.int32))
    need = int(((cl.cpu() + (T if lens is None else l32.cpu()) + _lib.KV_PAGE_TOKENS - 1) // _lib.KV_PAGE_TOKENS).max())
    if need > pt.shape[1]:
        raise RuntimeError(f"attention_paged: a row needs {need} pages, the table has {pt.shape[1]}")
    if out is None:
        out = (torch.empty(tiled_floats(B * T, Cd), dtype=torch.float32, device=qkv.device) if tiled
               else torch.empty(B, T, Cd, dtype=torch.float32, device=qkv.device))
    else:
        _buf(out, tiled_floats(B * T, Cd) if tiled else B * T * Cd, torch.float32, "attention_paged: out")
    part = count = None
    if scratch is not None:
        part, count = scratch
        _buf(part, 1, torch.float32, "attention_paged: scratch part")
        _buf(count, 1, torch.int32, "attention_paged: scratch count")
    io = (C.c_int32 * 1)(-1)
    fn = lib.mgea_op_attention_paged_causal if causal else lib.mgea_op_attention_paged_ex
    check(fn(ptr(qkv), ptr(pages), n_pages, int(n_layer), int(layer),
             _lib.DTYPE_F16 if pages.dtype == torch.float16 else _lib.DTYPE_F32, int(arith_batch), ptr(pt),
             pt.shape[1], ptr(cl), ptr(l32), ptr(out), B, T, n_head, dh, int(bool(tiled)), int(not split),
             ptr(part), 0 if part is None else part.numel(), ptr(count), 0 if count is None else count.numel(),
             io, stream_ptr()))
    if info is not None:
        info[:] = [int(io[0])]
    return out


def attn_split_count(B: int, n_head: int, T: int, max_pages: int) -> int:
    """the launcher's choice of workgroups per (row, head, query) for a paged launch that has a split scratch (host arithmetic)"""
    return int(_lib.load().mgea_op_attn_split_count(int(B), int(n_head), int(T), int(max_pages)))


def attn_split_scratch(head_dim: int, device="cuda"):
    """-> (part, count): a split-context scratch for attention_paged(scratch=...) -- part [items, splits, head_dim + 2] fp32 filled
    with poison, count [items] int32 ZERO (the one zeroing the kernel's contract asks for)."""
    pf, ci = C.c_int64(0), C.c_int64(0)
    check(_lib.load().mgea_op_attn_split_scratch(int(head_dim), C.byref(pf), C.byref(ci)))
    part = poison(pf.value, device=device).view(ci.value, -1, int(head_dim) + 2)
    return part, torch.zeros(ci.value, dtype=torch.int32, device=device)


def window_evict(page_table: torch.Tensor, sink_pages: int, ring_pages: int, ctx_len: torch.Tensor, done: torch.Tensor,
                 evictions: torch.Tensor):
    """The kernel that opens a windowed decode step (mgea_op_window_evict), alone: int32 copies of page_table [B, max_pages], ctx_len,
    done and evictions [B] (host or device tensors) on the device; returns the (page_table, ctx_len, evictions) it leaves there.  The
    host model of it: mgea.decoder.KVWindow.evict_rows."""
    lib = _lib.load()
    pt, cl, dn, ev = (t.to(device="cuda", dtype=torch.int32).contiguous().clone() for t in (page_table, ctx_len, done, evictions))
    if pt.dim() != 2 or any(t.shape != (pt.shape[0],) for t in (cl, dn, ev)):
        raise RuntimeError("window_evict: page_table must be [B, max_pages] and ctx_len / done / evictions [B]")
    check(lib.mgea_op_window_evict(ptr(pt), pt.shape[1], int(sink_pages), int(ring_pages), ptr(cl), ptr(dn), ptr(ev), pt.shape[0],
                                   stream_ptr()))
    return pt, cl, ev


def recondition(pool: torch.Tensor, store: torch.Tensor, lens, page_table=None, gather_seg: int = -1, schedules=None, done=None,
                row_step=None, gram_state=None, cur_seg=None):
    """The two kernels of a scheduled generation (mgea_op_recondition), alone, on COPIES of a KV pool [n_layer, n_pages, 2, H, 64 * dh]
    (fp32 or fp16, the page layouts of csrc/common.h) and of a conditioning store [n_seg_max, n_layer, B, 2 * H * dh * slot_tokens] of
    the pool's dtype.  lens: the B rows' prompt lengths (1 .. slot_tokens).  page_table None: row b's page is physical page b (the
    decoder's allocation rule); else int32 [B, max_pages], column 0 = the rows' pages.  gather_seg >= 0: the rows' positions
    [0, len) -> the slots of that segment.  schedules (B mgea.decoder.RowSchedule, or None = no apply): then one scheduled step's rule
    over done / row_step / gram_state / cur_seg (B ints each; default 0, gram_state -1).  Returns (pool, store, cur_seg, switches)
    as the launches leave them.  Sizes are checked here (the kernels trust them): RuntimeError."""
    lib = _lib.load()
    if pool.dim() != 5 or pool.shape[2] != 2 or pool.dtype not in (torch.float32, torch.float16) or store.dim() != 4 or store.dtype != pool.dtype:
        raise RuntimeError("recondition: pool must be [n_layer, n_pages, 2, H, 64 * dh] and store [n_seg_max, n_layer, B, slot] of one dtype (f32 / f16)")
    L, n_pages, _, H, pe = pool.shape
    dh = pe // _lib.KV_PAGE_TOKENS
    lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    B = len(lens)
    n_seg_max = store.shape[0]
    slot_tokens = store.shape[3] // (2 * H * dh) if dh else 0
    if pe != dh * _lib.KV_PAGE_TOKENS or store.shape[1] != L or store.shape[2] != B or B < 1 or store.shape[3] != 2 * H * dh * slot_tokens:
        raise RuntimeError(f"recondition: store {list(store.shape)} does not fit pool {list(pool.shape)} and {B} rows")
    if any(not 1 <= v <= min(slot_tokens, _lib.KV_PAGE_TOKENS) for v in lens):
        raise RuntimeError(f"recondition: lens {lens} outside [1, {slot_tokens}]")
    pl = pool.to("cuda").contiguous().clone()
    stc = store.to("cuda").contiguous().clone()
    pt = None
    if page_table is not None:
        pt = torch.as_tensor(page_table).to(device="cuda", dtype=torch.int32).contiguous()
        if pt.dim() != 2 or pt.shape[0] != B or int(pt[:, 0].min()) < 0 or int(pt[:, 0].max()) >= n_pages:
            raise RuntimeError("recondition: page_table must be [B, max_pages] with column 0 inside the pool")
    elif B > n_pages:
        raise RuntimeError(f"recondition: {B} rows but {n_pages} pages")

    def vec(v, default):
        v = [default] * B if v is None else [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
        if len(v) != B:
            raise RuntimeError(f"recondition: a vector of {len(v)} values for {B} rows")
        return torch.tensor(v, dtype=torch.int32, device="cuda")
    dn, rs, gs, cs = vec(done, 0), vec(row_step, 0), vec(gram_state, -1), vec(cur_seg, 0)
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ln_out = ln.clone()   # (the gather files the lengths it read here; the apply reads them)
    meta = torch.tensor([slot_tokens, B, n_seg_max, 0], dtype=torch.int32, device="cuda")
    sw = torch.zeros(4, dtype=torch.int32, device="cuda")
    sched = None
    if schedules is not None:
        schedules = list(schedules)
        if len(schedules) != B:
            raise RuntimeError(f"recondition: {len(schedules)} schedules for {B} rows")
        recs = (_lib.RowSchedule * B)(*[s.record() for s in schedules])
        sched = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.int32).to("cuda")
    check(lib.mgea_op_recondition(ptr(pl), L, n_pages, H, dh, int(pool.dtype == torch.float16), 0 if pt is not None else n_pages, ptr(pt),
                                  1 if pt is None else pt.shape[1], ptr(stc), n_seg_max, slot_tokens, ptr(meta), ptr(ln_out), B,
                                  int(gather_seg), ptr(ln), ptr(sched), ptr(dn), ptr(rs), ptr(gs), ptr(cs), ptr(sw), stream_ptr()))
    torch.cuda.synchronize()
    return pl, stc, cs, int(sw[0])


def guidance_mix(logits: torch.Tensor, partner, scale) -> torch.Tensor:
    """The mix launch of a guided decode step (mgea_op_guidance_mix), alone, on a COPY of logits [>= B, V] (B = len(partner); rows
    behind B are guard rows the kernel must not touch): for every row c with u = partner[c] >= 0, both rows become
    scale[c] * log_softmax(row c) + (1 - scale[c]) * log_softmax(row u).  partner / scale: B ints (-1 = not conditional) and B floats,
    checked on the host like a guided call's pairs (mgea.decoder.check_guidance: ValueError naming the row).  Returns the copy."""
    from .decoder import check_guidance
    lib = _lib.load()
    partner = [int(v) for v in (partner.tolist() if hasattr(partner, "tolist") else partner)]
    scale = [float(v) for v in (scale.tolist() if hasattr(scale, "tolist") else scale)]
    B = len(partner)
    if logits.dim() != 2 or logits.shape[0] < B or len(scale) != B or B < 1:
        raise RuntimeError("guidance_mix: logits must be [>= B, V] with B = len(partner) = len(scale) >= 1")
    check_guidance(partner, scale, B)
    out = logits.to(device="cuda", dtype=torch.float32).contiguous().clone()
    p = torch.tensor(partner, dtype=torch.int32, device="cuda")
    s = torch.tensor(scale, dtype=torch.float32, device="cuda")
    check(lib.mgea_op_guidance_mix(ptr(out), B, out.shape[1], ptr(p), ptr(s), stream_ptr()))
    return out


def blend_mix(logits: torch.Tensor, leader, weight) -> torch.Tensor:
    """The mix launch of a blended decode step (mgea_op_blend_mix), alone, on a COPY of logits [>= B, V] (B = len(leader); rows behind
    B are guard rows the kernel must not touch): the rows b with leader[b] == L, in ascending order, all become
    sum_k weight[m_k] * log_softmax(row m_k).  leader / weight: B ints (-1 = in no group) and B floats, checked on the host like a
    blended call's groups (mgea.decoder.check_blend: ValueError naming the row).  Returns the copy."""
    from .decoder import check_blend
    lib = _lib.load()
    leader = [int(v) for v in (leader.tolist() if hasattr(leader, "tolist") else leader)]
    weight = [float(v) for v in (weight.tolist() if hasattr(weight, "tolist") else weight)]
    B = len(leader)
    if logits.dim() != 2 or logits.shape[0] < B or len(weight) != B or B < 1:
        raise RuntimeError("blend_mix: logits must be [>= B, V] with B = len(leader) = len(weight) >= 1")
    check_blend(leader, weight, B)
    out = logits.to(device="cuda", dtype=torch.float32).contiguous().clone()
    l = torch.tensor(leader, dtype=torch.int32, device="cuda")
    w = torch.tensor(weight, dtype=torch.float32, device="cuda")
    check(lib.mgea_op_blend_mix(ptr(out), B, out.shape[1], ptr(l), ptr(w), stream_ptr()))
    return out


def class_penalty(logits: torch.Tensor, class_of, hist, row_step, done, recs) -> torch.Tensor:
    """The class-penalty launch of a class-penalised decode step (mgea_op_class_penalty), alone, on a COPY of logits [>= B, V] (B =
    len(recs); rows behind B are guard rows the kernel must not touch).  class_of: V ints in [-1, n_class), n_class = the largest
    class + 1 (at least 1); hist: int [B, stride], row b's taken ids; row_step / done: B ints; recs: B mgea.decoder.ClassPenalty
    (checked on the host: ValueError naming the row).  Returns the copy."""
    lib = _lib.load()
    recs = list(recs)
    B = len(recs)
    hist = torch.as_tensor(hist, dtype=torch.int32)
    class_of = torch.as_tensor(class_of, dtype=torch.int32)
    row_step = torch.as_tensor(row_step, dtype=torch.int32)
    done = torch.as_tensor(done, dtype=torch.int32)
    if logits.dim() != 2 or logits.shape[0] < B or B < 1 or hist.dim() != 2 or hist.shape[0] != B or hist.shape[1] < 1:
        raise RuntimeError("class_penalty: logits must be [>= B, V] and hist [B, stride >= 1] with B = len(recs) >= 1")
    V = logits.shape[1]
    if class_of.dim() != 1 or class_of.shape[0] != V or row_step.shape != (B,) or done.shape != (B,):
        raise RuntimeError("class_penalty: class_of must be [V], row_step and done [B]")
    if int(row_step.max()) > hist.shape[1] or int(row_step.min()) < 0:
        raise ValueError(f"class_penalty: row_step outside [0, stride = {hist.shape[1]}]")
    if int(class_of.min()) < -1:
        raise ValueError("class_penalty: class_of below -1")
    n_class = max(int(class_of.max()) + 1, 1)
    for b, r in enumerate(recs):
        r.check(b)
    crecs = (_lib.RowClassPenalty * B)(*[r.record() for r in recs])
    out = logits.to(device="cuda", dtype=torch.float32).contiguous().clone()
    dev = [t.to("cuda").contiguous() for t in (class_of, hist, row_step, done)]
    check(lib.mgea_op_class_penalty(ptr(out), B, V, ptr(dev[0]), n_class, ptr(dev[1]), hist.shape[1], ptr(dev[2]), ptr(dev[3]), crecs,
                                    stream_ptr()))
    return out


# ---- the DistilBERT row, [CLS] and split-K epilogue kernels, one launch per call (mgea_op_* of the same names: tests only) ----
_DTYPE_ROWS = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}


def _i32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else _dev(t.to(torch.int32))


def _rows2d(t: torch.Tensor, what: str) -> torch.Tensor:
    """a device fp32 [rows, cols] view whose columns are contiguous (the row stride is the leading dimension the kernel gets)"""
    if t.device.type != "cuda" or t.dtype != torch.float32 or t.ndim != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{what}: an fp32 device matrix with contiguous columns is needed")
    return t


def attention_cls(q: torch.Tensor, qkv: torch.Tensor, n_head: int, mask: Optional[torch.Tensor] = None,
                  cu: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The [CLS] attention (mgea_op_attention_cls): q [B, D] fp32, one query per sequence; qkv [B, S, 3 D] (padded; mask [B, S] or
    None) or [cu[B], 3 D] with cu [B + 1] (packed), fp32 or bf16 (only its K | V columns are read) -> [B, D] fp32."""
    lib = _lib.load()
    if qkv.dtype not in _DTYPE_ROWS:
        raise RuntimeError("attention_cls takes an fp32 or bf16 qkv")
    q, qkv = _dev(q.float()), _dev(qkv)
    B, D = q.shape
    if qkv.shape[-1] != 3 * D or D % n_head:
        raise RuntimeError("attention_cls: qkv rows hold 3 D columns, D = n_head * head_dim")
    c32 = _i32(cu)
    if cu is not None:
        if qkv.ndim != 2 or cu.numel() != B + 1 or int(cu[-1]) != qkv.shape[0] or int(cu[0]) != 0 or bool((cu[1:] < cu[:-1]).any()):
            raise RuntimeError("packed attention_cls: qkv must be [cu[B], 3 D] and cu [B + 1] non-decreasing from 0")
        S = 0
    else:
        if qkv.ndim != 3 or qkv.shape[0] != B:
            raise RuntimeError("attention_cls: qkv must be [B, S, 3 D]")
        S = qkv.shape[1]
    m32 = _i32(mask)
    if m32 is not None and cu is None and tuple(m32.shape) != (B, S):
        raise RuntimeError("attention_cls: mask must be [B, S]")
    out = torch.full((B, D), float("nan"), dtype=torch.float32, device=q.device)
    check(lib.mgea_op_attention_cls(ptr(q), ptr(qkv), _DTYPE_ROWS[qkv.dtype], ptr(m32), ptr(c32), ptr(out), B, S, n_head, D // n_head,
                                    stream_ptr()))
    return out


def bert_embed(ids: torch.Tensor, word: torch.Tensor, pos: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, eps: float,
               out_dtype: torch.dtype = torch.float32, pos_ids: Optional[torch.Tensor] = None, want_flag: bool = True,
               out: Optional[torch.Tensor] = None):
    """LayerNorm(word[ids] + pos[t]) by the DistilBERT embedding kernel (mgea_op_bert_embed): ids [B, S] (t = the column), or [rows]
    with pos_ids [rows] (packed).  -> (out [rows, D] fp32 or bf16, flag): flag = the error word after the call (1: an id was clamped), None
    with want_flag=False (the kernel then gets no flag word).  out: the caller's buffer (left as it is when the call is refused)."""
    lib = _lib.load()
    word, pos, ln_w, ln_b = (_dev(t.float()) for t in (word, pos, ln_w, ln_b))
    ids = _i32(ids)
    p32 = _i32(pos_ids)
    if p32 is not None:
        if ids.ndim != 1 or p32.shape != ids.shape:
            raise RuntimeError("packed bert_embed: ids and pos_ids are [rows]")
        B, S, tmax = ids.numel(), 1, int(p32.max())
        if int(p32.min()) < 0:
            raise RuntimeError("bert_embed: negative position")
    else:
        B, S = ids.shape
        tmax = S - 1
    V, D = word.shape
    if pos.shape[1] != D or pos.shape[0] <= tmax or ln_w.numel() != D or ln_b.numel() != D:
        raise RuntimeError("bert_embed: pos must be [> every position, D], ln_w and ln_b [D]")
    if out is None:
        out = torch.empty(B * S, D, dtype=out_dtype, device=ids.device)
    if out.dtype != out_dtype or out.numel() < B * S * D or not out.is_contiguous() or out_dtype not in _DTYPE_ROWS:
        raise RuntimeError("bert_embed: out must be a contiguous fp32 or bf16 tensor of rows * D elements")
    flag = torch.zeros(1, dtype=torch.int32, device=ids.device) if want_flag else None
    check(lib.mgea_op_bert_embed(ptr(ids), ptr(p32), ptr(word), ptr(pos), ptr(ln_w), ptr(ln_b), float(eps), ptr(out), _DTYPE_ROWS[out_dtype],
                                 B, S, D, V, ptr(flag), stream_ptr()))
    return out, (int(flag.item()) if want_flag else None)


def gather_cls(h: torch.Tensor, B: int, S: int, cu: Optional[torch.Tensor] = None, rowstat: Optional[torch.Tensor] = None,
               ln_g: Optional[torch.Tensor] = None, ln_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The [CLS] rows of h [rows, D] (fp32 or bf16) -> [B, D] fp32 (mgea_op_gather_cls): row b S, or row cu[b] with cu [B + 1].  bf16
    with rowstat [rows, 2] = (mean, rstd): the folded LayerNorm ((h - mean) rstd) ln_g + ln_b of those rows."""
    lib = _lib.load()
    if h.dtype not in _DTYPE_ROWS or h.ndim != 2:
        raise RuntimeError("gather_cls takes an fp32 or bf16 [rows, D] matrix")
    h = _dev(h)
    rows, D = h.shape
    c32 = _i32(cu)
    first = [int(c) for c in cu[:B]] if cu is not None else [b * S for b in range(B)]
    if (cu is not None and cu.numel() != B + 1) or min(first) < 0 or max(first) >= rows:
        raise RuntimeError("gather_cls: a [CLS] row lies outside h")
    rs = None if rowstat is None else _dev(rowstat.float())
    if rs is not None and rs.numel() != rows * 2:
        raise RuntimeError("gather_cls: rowstat must be [rows, 2]")
    g = None if ln_g is None else _dev(ln_g.float())
    be = None if ln_b is None else _dev(ln_b.float())
    out = torch.full((B, D), float("nan"), dtype=torch.float32, device=h.device)
    check(lib.mgea_op_gather_cls(ptr(h), _DTYPE_ROWS[h.dtype], ptr(rs), ptr(g), ptr(be), ptr(c32), ptr(out), B, S, D, stream_ptr()))
    return out


def gemm_direct(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, act: int = 0) -> torch.Tensor:
    """The fp32 GEMM with its bias / activation epilogue inside the kernel (mgea_op_gemm_f32_direct): out[:, :] = act(a w^T + bias),
    written in place.  a [M, K], w [N, K] and out [M, N] are device VIEWS with contiguous columns: their row strides go to the kernel as
    lda / ldw / ldo, so a column slice of a wider matrix is read or written in place."""
    lib = _lib.load()
    a, w, out = _rows2d(a, "gemm_direct a"), _rows2d(w, "gemm_direct w"), _rows2d(out, "gemm_direct out")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(out.shape) != (M, N):
        raise RuntimeError("gemm_direct: a [M, K], w [N, K], out [M, N]")
    b = None if bias is None else _dev(bias.float())
    if b is not None and b.numel() != N:
        raise RuntimeError("gemm_direct: bias [N]")
    check(lib.mgea_op_gemm_f32_direct(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(b), ptr(out), out.stride(0), M, N, K, int(act),
                                      stream_ptr()))
    return out


def _slabs(P: torch.Tensor, what: str):
    """P [S, M, ldp] fp32 on the device, rows contiguous -> (S, slab stride, ldp, M)"""
    if P.device.type != "cuda" or P.dtype != torch.float32 or P.ndim != 3 or P.stride(2) != 1 or P.stride(1) != P.shape[2]:
        raise RuntimeError(f"{what}: the slabs are an fp32 device tensor [S, M, ldp] with contiguous rows")
    return P.shape[0], (P.stride(0) if P.shape[0] > 1 else 0), P.shape[2], P.shape[1]


def slab_bias_act(P: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, act: int = 0) -> torch.Tensor:
    """out[m, n] = act(sum_s P[s, m, n] + bias[n]) (mgea_op_slab_bias_act), in place: out is a device view [M, N] with contiguous
    columns whose row stride is the kernel's ldo."""
    lib = _lib.load()
    S, ps, ldp, M = _slabs(P, "slab_bias_act")
    out = _rows2d(out, "slab_bias_act out")
    N = out.shape[1]
    b = None if bias is None else _dev(bias.float())
    if out.shape[0] != M or (b is not None and b.numel() < N):
        raise RuntimeError("slab_bias_act: out [M, N], bias [N]")
    check(lib.mgea_op_slab_bias_act(ptr(P), S, ps, ldp, ptr(b), ptr(out), out.stride(0), M, N, int(act), stream_ptr()))
    return out


def slab_bias_res_ln(P: torch.Tensor, bias: Optional[torch.Tensor], x: torch.Tensor, ln_w: Optional[torch.Tensor] = None,
                     ln_b: Optional[torch.Tensor] = None, eps: float = 1e-5, post_ln: bool = False):
    """The residual / LayerNorm epilogue (mgea_op_slab_bias_res_ln) on x [M, C] (contiguous fp32 device tensor, updated in place):
    pre-LN x += v and xn = LN(x) when ln_w is given; post-LN x = LN(x + v).  Returns (x, xn or None)."""
    lib = _lib.load()
    S, ps, ldp, M = _slabs(P, "slab_bias_res_ln")
    if x.device.type != "cuda" or x.dtype != torch.float32 or x.ndim != 2 or not x.is_contiguous() or x.shape[0] != M:
        raise RuntimeError("slab_bias_res_ln: x is a contiguous fp32 device tensor [M, C]")
    Cd = x.shape[1]
    b = None if bias is None else _dev(bias.float())
    w = None if ln_w is None else _dev(ln_w.float())
    be = None if ln_b is None else _dev(ln_b.float())
    if any(t is not None and t.numel() < Cd for t in (b, w, be)):
        raise RuntimeError("slab_bias_res_ln: bias, ln_w and ln_b are [C]")
    xn = torch.full_like(x, float("nan")) if (w is not None and not post_ln) else None
    check(lib.mgea_op_slab_bias_res_ln(ptr(P), S, ps, ldp, ptr(b), ptr(x), ptr(xn), ptr(w), ptr(be), float(eps), M, Cd, int(bool(post_ln)),
                                       stream_ptr()))
    return x, xn


def slab_logits_argmax(P: torch.Tensor, bias: Optional[torch.Tensor], V: int, logits: Optional[torch.Tensor] = None,
                       argmax: Optional[torch.Tensor] = None):
    """logits [M, V] = sum_s P[s] + bias and argmax [M] int32 = the lowest index of each row's maximum (mgea_op_slab_logits_argmax);
    each output is written only if its (contiguous device) buffer is passed.  Returns (logits, argmax) as passed."""
    lib = _lib.load()
    S, ps, ldp, M = _slabs(P, "slab_logits_argmax")
    b = None if bias is None else _dev(bias.float())
    if ldp < V or (b is not None and b.numel() < V):
        raise RuntimeError("slab_logits_argmax: ldp >= V, bias [V]")
    if logits is not None and (logits.dtype != torch.float32 or logits.numel() < M * V or not logits.is_contiguous() or logits.device != P.device):
        raise RuntimeError("slab_logits_argmax: logits must be a contiguous fp32 device tensor [M, V]")
    if argmax is not None and (argmax.dtype != torch.int32 or argmax.numel() < M or not argmax.is_contiguous() or argmax.device != P.device):
        raise RuntimeError("slab_logits_argmax: argmax must be a contiguous int32 device tensor [M]")
    check(lib.mgea_op_slab_logits_argmax(ptr(P), S, ps, ldp, ptr(b), ptr(logits), M, int(V), ptr(argmax), stream_ptr()))
    return logits, argmax


def slab_qkv_scatter(P: torch.Tensor, bias: Optional[torch.Tensor], n_head: int, head_dim: int, pages: torch.Tensor,
                     page_table: torch.Tensor, ctx_len: torch.Tensor, lens: Optional[torch.Tensor], T: int, want_qkv: bool = True):
    """The qkv epilogue with its KV-page scatter (mgea_op_slab_qkv_scatter).  P [S, B T, ldp]; pages: one layer of device KV pages (fp32
    or fp16), written in place at positions ctx_len[b] + t, t < lens[b].  want_qkv: qkv_out [B T, 3 C] = the slab sum + bias (zero rows
    past lens) is returned; False: scatter only, P[0] is the finished buffer and nothing else is written."""
    lib = _lib.load()
    S, ps, ldp, M = _slabs(P, "slab_qkv_scatter")
    Cd = n_head * head_dim
    if pages.dtype not in (torch.float32, torch.float16) or not pages.is_contiguous() or pages.device != P.device:
        raise RuntimeError("slab_qkv_scatter: pages must be a contiguous fp32 or fp16 device tensor")
    n_pages = pages.numel() // kv_page_elems(1, n_head, head_dim)
    pt, cl, l32 = _i32(page_table), _i32(ctx_len), _i32(lens)
    B = M // T
    if M % T or pt.ndim != 2 or pt.shape[0] != B or cl.shape != (B,) or (l32 is not None and l32.shape != (B,)) or ldp < 3 * Cd:
        raise RuntimeError("slab_qkv_scatter: P [S, B T, >= 3 C], page_table [B, max_pages], ctx_len and lens [B]")
    if n_pages < 1 or int(pt.min()) < 0 or int(pt.max()) >= n_pages or int(cl.min()) < 0:
        raise RuntimeError("slab_qkv_scatter: page table entries must lie in [0, n_pages), context lengths must not be negative")
    b = None if bias is None else _dev(bias.float())
    if b is not None and b.numel() < 3 * Cd:
        raise RuntimeError("slab_qkv_scatter: bias [3 C]")
    out = torch.full((M, 3 * Cd), float("nan"), dtype=torch.float32, device=P.device) if want_qkv else None
    check(lib.mgea_op_slab_qkv_scatter(ptr(P), S, ps, ldp, ptr(b), ptr(out), ptr(pages), n_pages,
                                       _lib.DTYPE_F16 if pages.dtype == torch.float16 else _lib.DTYPE_F32, ptr(pt), pt.shape[1], ptr(cl),
                                       ptr(l32), B, T, n_head, head_dim, stream_ptr()))
    return out


def lora_merge(w: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float) -> torch.Tensor:
    """W [out, in] + scale * B [out, r] @ A [r, in] by the LoRA fold kernel (mgea_lora_merge) -> a new [out, in] fp32 tensor."""
    lib = _lib.load()
    w, a, b = _dev(w.float()).clone(), _dev(a.float()), _dev(b.float())
    out_dim, in_dim = w.shape
    r = a.shape[0]
    if tuple(a.shape) != (r, in_dim) or tuple(b.shape) != (out_dim, r):
        raise RuntimeError("lora_merge: W [out, in], A [r, in], B [out, r]")
    check(lib.mgea_lora_merge(ptr(w), ptr(a), ptr(b), out_dim, in_dim, r, float(scale), stream_ptr()))
    return w


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


def _sampler_inputs(logits: torch.Tensor, rows, presence, presence_alone: bool, forced=None, grammar=None, states=None):
    """The front half of the row samplers (sample_rows, sample_rows_scored, sample_rows_grammar, sample_rows_truncated): the logits on
    the device, the rows' sampler records (one per logits row), the presence words -- passed when a row's penalty is not 1 and, with
    presence_alone, whenever presence is given --, the rows' logit records (with the tensors they point into: keep them until the call
    has been made), the forced ids as an int32 [B] vector and the grammar's tables with the rows' states in and out, None for what the
    call has not.  Returns (logits, recs, bits, lrecs, keep, forced, (class_of, next, states_in, states_out))."""
    from .decoder import pack_row_logits, pack_rows
    logits = _dev(logits.float())
    B, V = logits.shape
    dev = logits.device
    if grammar is not None:
        grammar.check(V)
    recs = pack_rows(rows, V)
    if len(recs) != B:
        raise ValueError(f"{B} logits rows but {len(recs)} sampler rows")
    bits = None
    if (presence_alone and presence is not None) or any(r.repetition_penalty != 1.0 for r in recs):
        words = pack_presence(presence if presence is not None else [[] for _ in range(B)], B, V)
        bits = torch.from_numpy(words.view(np.int32)).to(dev)
    lrecs, keep = pack_row_logits(rows, V, dev)
    if forced is not None:
        forced = torch.as_tensor(forced).to(device=dev, dtype=torch.int32).contiguous()
        if forced.shape != (B,):
            raise ValueError(f"forced must hold {B} ids, got {list(forced.shape)}")
    tables = (None, None, None, None)
    if grammar is not None:
        st = np.asarray(list(states), dtype=np.int64).reshape(-1)
        if st.shape != (B,) or st.min() < -1 or st.max() >= grammar.n_state:
            raise ValueError(f"states must be {B} values in [-1, {grammar.n_state})")
        tables = (torch.from_numpy(grammar.class_of).to(dev), torch.from_numpy(grammar.next).to(dev),
                  torch.from_numpy(st.astype(np.int32)).to(dev), torch.empty(B, dtype=torch.int32, device=dev))
    return logits, recs, bits, lrecs, keep, forced, tables


def _sample_rows(logits: torch.Tensor, rows, step, want_probs, presence, logit_bias, min_new_tokens, scored, forced):
    """sample_rows / sample_rows_scored: pack the rows, one native call."""
    import dataclasses
    from .decoder import split_logit_bias
    rows = list(rows)
    if logit_bias is not None or min_new_tokens is not None:
        nb = len(rows)
        per_row = split_logit_bias(logit_bias, nb)
        mins = list(min_new_tokens) if isinstance(min_new_tokens, (list, tuple)) else [min_new_tokens] * nb
        rows = [dataclasses.replace(r, logit_bias=r.logit_bias if logit_bias is None else per_row[b],
                                    min_new_tokens=r.min_new_tokens if mins[b] is None else int(mins[b]))
                for b, r in enumerate(rows)]
    lib = _lib.load()
    logits, recs, bits, lrecs, keep, f, _ = _sampler_inputs(logits, rows, presence, False, forced if scored else None)
    B, V = logits.shape
    ids = torch.empty(B, dtype=torch.int32, device=logits.device)
    probs = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_probs else None
    if scored:
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


def sample_rows_grammar(logits: torch.Tensor, rows, grammar, states, step=0, want_probs=False, presence=None):
    """sample_rows() under a mgea.decoder.TokenGrammar (mgea_op_sample_rows_grammar): row b in state states[b] (-1 = no grammar on
    the row) loses every id its state bans -- after its penalty and bias, before the EOS ban -- and moves to
    grammar.step(states[b], id).  The rows' own logit_bias / min_new_tokens apply.  Returns (ids, states_out[, probs])."""
    lib = _lib.load()
    logits, recs, bits, lrecs, keep, _, (cls, nxt, s_in, s_out) = _sampler_inputs(logits, list(rows), presence, True, None, grammar, states)
    B, V = logits.shape
    ids = torch.empty(B, dtype=torch.int32, device=logits.device)
    probs = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_probs else None
    check(lib.mgea_op_sample_rows_grammar(ptr(logits), B, V, recs, ptr(bits), lrecs, ptr(cls), ptr(nxt), grammar.n_state, grammar.n_class,
                                          ptr(s_in), int(step), ptr(ids), ptr(probs), ptr(s_out), stream_ptr()))
    return (ids, s_out, probs) if want_probs else (ids, s_out)


def sample_rows_truncated(logits: torch.Tensor, rows, truncation=None, step=0, want_probs=False, presence=None, scored=False,
                          forced=None, grammar=None, states=None):
    """sample_rows() through the truncating sampler (mgea_op_sample_rows_truncated): behind temperature, top-k and top-p, row b applies
    min-p, typical-p, the epsilon and the eta cutoff of its mgea.decoder.Truncation, in this order (include/mgea.h,
    mgea_row_truncation).  truncation: None = the rows' own `truncation` attributes, one Truncation for every row, or one (or None)
    per row; with none anywhere this is the op it extends.  scored / forced as in sample_rows_scored, grammar / states as in
    sample_rows_grammar, in any combination.  Returns ids, then (logprobs, choice_logprobs) if scored, then states_out if a grammar
    is given, then probs if want_probs -- a tuple unless ids stands alone."""
    import dataclasses
    from .decoder import Truncation, pack_truncation
    rows = list(rows)
    if truncation is not None:
        per = [truncation] * len(rows) if isinstance(truncation, Truncation) else list(truncation)
        if len(per) != len(rows):
            raise ValueError(f"{len(rows)} sampler rows but {len(per)} truncation records")
        rows = [dataclasses.replace(r, truncation=t) for r, t in zip(rows, per)]
    if forced is not None and not scored:
        raise ValueError("forced ids need scored=True")
    lib = _lib.load()
    logits, recs, bits, lrecs, keep, f, (cls, nxt, s_in, s_out) = _sampler_inputs(logits, rows, presence, True, forced, grammar, states)
    B, V = logits.shape
    dev = logits.device
    trecs = pack_truncation(rows)
    ids = torch.empty(B, dtype=torch.int32, device=dev)
    probs = torch.empty(B, V, dtype=torch.float32, device=dev) if want_probs else None
    lp = torch.empty(B, dtype=torch.float32, device=dev) if scored else None
    ch = torch.empty(B, dtype=torch.float32, device=dev) if scored else None
    n_state, n_class = (grammar.n_state, grammar.n_class) if grammar is not None else (0, 0)
    check(lib.mgea_op_sample_rows_truncated(ptr(logits), B, V, recs, ptr(bits), lrecs, trecs, int(step), ptr(ids), ptr(probs), ptr(f), ptr(lp),
                                            ptr(ch), ptr(cls), ptr(nxt), n_state, n_class, ptr(s_in), ptr(s_out), stream_ptr()))
    out = (ids,) + ((lp, ch) if scored else ()) + ((s_out,) if grammar is not None else ()) + ((probs,) if want_probs else ())
    return out[0] if len(out) == 1 else out


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


# ---- the decode-step GEMMs one plan at a time (mgea_op_decode_gemm: tests only) ----
POISON_BITS = 0x7FC5A5A5   # a quiet NaN no kernel produces: buffers pre-filled with it show, compared as int32, what was written
PLAN_KEYS = ("kind", "mt", "nt", "nw", "nch", "cw", "mr", "base", "grid_x", "grid_y", "n_partials")


def poison(n, dtype=torch.float32, device="cpu") -> torch.Tensor:
    """n elements of `dtype` (fp32 or fp16) whose bits are POISON_BITS (fp16: its upper half, also a NaN)"""
    if dtype == torch.float16:
        return torch.full((int(n),), POISON_BITS >> 16, dtype=torch.int16, device=device).view(torch.float16)
    return torch.full((int(n),), POISON_BITS, dtype=torch.int32, device=device).view(torch.float32)


def tile_weights_f16(w: torch.Tensor) -> torch.Tensor:
    """W [N,K] row-major fp32 -> the fp16 fragments the fp16-weight decode GEMMs read (rows padded to 32 with zeros)."""
    lib = _lib.load()
    w = _dev(w.float())
    N, K = w.shape
    out = torch.empty(lib.mgea_op_tiled_weight_floats(N, K), dtype=torch.float16, device=w.device)
    check(lib.mgea_op_tile_weights_f16(ptr(w), N, K, ptr(out), stream_ptr()))
    return out


def ln_vectors(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """(c1 [N] = sum_k gamma[k] w[n,k], c2 [N] = sum_k beta[k] w[n,k] + bias[n]) of the folded LayerNorm with gamma on the
    activation side (fp16 weights): w is the matrix the kernel multiplies with, i.e. already rounded to fp16 values."""
    lib = _lib.load()
    w, gamma, beta = _dev(w.float()), _dev(gamma.float()), _dev(beta.float())
    b = None if bias is None else _dev(bias.float())
    N, K = w.shape
    c1 = torch.empty(N, dtype=torch.float32, device=w.device)
    c2 = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib.mgea_op_ln_vectors(ptr(w), ptr(gamma), ptr(beta), ptr(b), N, K, ptr(c1), ptr(c2), stream_ptr()))
    return c1, c2


def decode_gemm(epi: int, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], M: int, N: int, K: int, *,
                rowmajor: bool = False, w_f16: bool = False, act: int = 0, eps: float = 1e-5, ln_c1=None, ln_g=None, ln_b=None,
                stats_in=None, part_cnt: int = 16, out=None, stats_out=None, kv: Optional[dict] = None, partials=None,
                want_out: bool = True):
    """One decode-step GEMM through mgea_op_decode_gemm on prepared device buffers: a = k-tiled activations (tile_rows), w = the
    row-major matrix (rowmajor), the tiled copy (tile_weights / fold_ln) or fp16 fragments (w_f16, tile_weights_f16).  epi 0 QKV
    (kv = dict(pages, n_pages, n_head, head_dim, layer, page_table [B, max_pages], ctx_len [B], lens=None, T=1, arith_batch=0 -- > 0: the
    pool carries the decoder's allocation rule, page j of row b = j * arith_batch + b, which the table must repeat); pages: the device
    image of >= layer + 1 layers, written in place), 1 RES (out = the k-tiled residual, updated in place), 2 ACT, 3 LOGITS.
    Buffers not passed are allocated: out (QKV / LOGITS row-major [M, N] filled with NaN, ACT k-tiled zeros), stats_out for RES,
    the LOGITS partials pre-filled with POISON_BITS.  Returns (out, extras, plan): extras holds stats_out [M, N / 16, 2] (RES) or
    partials = the raw buffer with R = max(64, M) and P = plan['n_partials'] (LOGITS: values [R][P] then indices [R][P], mgea.h);
    plan maps PLAN_KEYS to what ran.  A refused plan raises RuntimeError and launches nothing."""
    lib = _lib.load()
    dev = a.device
    g = _lib.DecodeGemmArgs()
    keep = [_dev(a), _dev(w)]
    if keep[0].dtype != torch.float32 or keep[1].dtype != (torch.float16 if w_f16 else torch.float32):
        raise RuntimeError("decode_gemm: a is fp32; w is fp32, or fp16 fragments with w_f16")
    if keep[0].numel() < (M + 63) // 64 * 64 * K or keep[1].numel() < (N * K if rowmajor else lib.mgea_op_tiled_weight_floats(N, K)):
        raise RuntimeError("decode_gemm: a or w is smaller than its layout needs")

    def f32(t, n=None):
        if t is None:
            return None
        t = _dev(t)
        if t.dtype != torch.float32 or (n is not None and t.numel() < n):
            raise RuntimeError("decode_gemm: an fp32 vector is too short or of another dtype")
        keep.append(t)
        return t

    g.epi, g.rowmajor, g.w_f16, g.M, g.N, g.K, g.act, g.eps = int(epi), int(bool(rowmajor)), int(bool(w_f16)), M, N, K, int(act), float(eps)
    g.a_dev, g.w_dev, g.bias_dev = ptr(keep[0]), ptr(keep[1]), ptr(f32(bias, N))
    g.ln_c1_dev, g.ln_g_dev, g.ln_b_dev = ptr(f32(ln_c1, N)), ptr(f32(ln_g, K)), ptr(f32(ln_b, K))
    if stats_in is not None:
        stats_in = f32(stats_in)
        if stats_in.ndim != 3 or stats_in.shape[0] < M or stats_in.shape[2] != 2:
            raise RuntimeError("decode_gemm: stats_in must be [M, n_part, 2]")
        g.stats_in_dev, g.n_part, g.part_cnt = ptr(stats_in), stats_in.shape[1], int(part_cnt)
    tiled = (M + 63) // 64 * 64 * N
    extras = {}
    if epi == _lib.EPI_RES:
        if out is None or out.numel() < tiled:
            raise RuntimeError("decode_gemm: RES updates the k-tiled residual `out` in place")
        if stats_out is None and not rowmajor:
            stats_out = torch.zeros(max(64, M) * (N // 16) * 2, dtype=torch.float32, device=dev)
    elif epi == _lib.EPI_ACT:
        if out is None:
            out = torch.zeros(tiled, dtype=torch.float32, device=dev)
        if out.numel() < tiled:
            raise RuntimeError("decode_gemm: ACT writes a k-tiled buffer of whole 64-row groups")
    elif out is None and (want_out or epi == _lib.EPI_QKV):
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device=dev)
    if out is not None and (out.dtype != torch.float32 or out.numel() < M * N or not out.is_contiguous()):
        raise RuntimeError("decode_gemm: out must be a contiguous fp32 tensor of at least M * N elements")
    g.out_dev = ptr(out)
    if stats_out is not None:
        if stats_out.numel() < M * (N // 16) * 2:
            raise RuntimeError("decode_gemm: stats_out holds [M, N / 16, 2]")
        g.stats_out_dev = ptr(f32(stats_out))
        extras["stats_out"] = stats_out[: M * (N // 16) * 2].view(M, N // 16, 2)
    if epi == _lib.EPI_QKV:
        pages, H, dh, layer, T = kv["pages"], int(kv["n_head"]), int(kv["head_dim"]), int(kv["layer"]), int(kv.get("T", 1))
        n_pages = int(kv["n_pages"])
        if pages.dtype not in (torch.float32, torch.float16) or not pages.is_contiguous() or pages.device != dev:
            raise RuntimeError("decode_gemm: pages must be a contiguous fp32 or fp16 device tensor")
        if layer < 0 or pages.numel() < (layer + 1) * kv_page_elems(n_pages, H, dh):
            raise RuntimeError("decode_gemm: the page image must hold layer + 1 layers of n_pages pages")
        pt = _dev(kv["page_table"].to(torch.int32))
        cl = _dev(kv["ctx_len"].to(torch.int32))
        l32 = None if kv.get("lens") is None else _dev(kv["lens"].to(torch.int32))
        if T < 1 or M % T or pt.ndim != 2 or pt.shape[0] != M // T or cl.shape != (M // T,) or (l32 is not None and l32.shape != cl.shape):
            raise RuntimeError("decode_gemm: page_table [M / T, max_pages], ctx_len and lens [M / T]")
        if int(pt.min()) < 0 or int(pt.max()) >= n_pages or int(cl.min()) < 0:
            raise RuntimeError("decode_gemm: page table entries must lie in [0, n_pages), context lengths must not be negative")
        keep += [pt, cl, l32]
        g.pages_dev, g.page_table_dev, g.ctx_len_dev, g.lens_dev = ptr(pages), ptr(pt), ptr(cl), ptr(l32)
        g.n_pages, g.page_dtype = n_pages, (_lib.DTYPE_F16 if pages.dtype == torch.float16 else _lib.DTYPE_F32)
        g.n_head, g.head_dim, g.layer, g.max_pages, g.T = H, dh, layer, pt.shape[1], T
        g.arith_batch = int(kv.get("arith_batch", 0))
    if epi == _lib.EPI_LOGITS:
        R = max(64, M)
        need = 2 * R * max((N + 15) // 16, 512)
        if partials is None:
            partials = poison(need + 64, device=dev)
        if partials.dtype != torch.float32 or partials.numel() < need:
            raise RuntimeError(f"decode_gemm: the partials buffer needs {need} floats")
        g.partials_dev = ptr(partials)
        extras.update(partials=partials, R=R)
    po = (C.c_int32 * _lib.DECODE_GEMM_PLAN_INTS)()
    check(lib.mgea_op_decode_gemm(C.byref(g), po, stream_ptr()))
    plan = dict(zip(PLAN_KEYS, (int(v) for v in po)))
    if epi == _lib.EPI_LOGITS:
        extras["P"] = plan["n_partials"]
    return out, extras, plan


def merge_partials(partials: torch.Tensor, M: int, R: int, P: int) -> torch.Tensor:
    """the greedy tail's merge of the (max, argmax) partials of rows < M: the lowest index among the partials that hold the row maximum"""
    p = partials.cpu()
    val = p[: R * P].view(R, P)[:M]
    idx = p[R * P: 2 * R * P].view(torch.int32).view(R, P)[:M].long()
    best = val.max(1, keepdim=True).values
    return torch.where(val == best, idx, torch.full_like(idx, 2 ** 31 - 1)).min(1).values


# ---- the kernels that end a decode step and the decoder's prefill row kernels, one launch per call (tests only) ----
def _buf(t: Optional[torch.Tensor], n: int, dtype, what: str) -> Optional[torch.Tensor]:
    """a caller buffer of an op_* call: on the device, contiguous, of `dtype`, at least n elements (None passes)"""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous() or t.dtype != dtype or t.numel() < int(n):
        raise RuntimeError(f"{what}: needs a contiguous {dtype} device tensor of at least {int(n)} elements")
    return t


def tiled_floats(M: int, N: int) -> int:
    """floats of a k-tiled [M, N] buffer: whole 64-row groups; a width that is no multiple of 32 leaves its last 32-wide k-chunk
    partly used, and such a buffer holds one row group only (the next group would start inside that chunk)"""
    if N % 32 == 0:
        return (M + 63) // 64 * 64 * N
    if M > 64:
        raise RuntimeError(f"a k-tiled buffer of width {N} (no multiple of 32) holds at most 64 rows")
    return 64 * ((N + 31) // 32 * 32)


def step_tail(kind: int, B: int, state: dict, *, rows=None, ctx_cap=None, eos_id: int = -1, partials=None, sampled=None, embed=None,
              table=None, presence=None, V: int = 0, scores=None, sampler=None, grammar=None, err_flag=None):
    """One end-of-step launch through mgea_op_step_tail (include/mgea.h) on caller buffers, all written in place.
    kind: _lib.TAIL_ARGMAX / TAIL_ARGMAX_EMBED / TAIL_ADVANCE / TAIL_EMBED_QKV0 / TAIL_SAMPLE.
    state   dict(cur_ids, ctx_len, done, row_step [>= B] int32, n_done [1], ids_out [B * n_steps] or None, n_steps)
    rows    None (the by-value eos_id, no budgets) or B mgea.decoder.RowSampling (max_new_tokens is not held to n_steps here);
            ctx_cap: None or B ints
    partials (pval fp32, pidx int32 [B * n_tiles], n_tiles); sampled int32 [B]
    embed   dict(tok_emb [vocab * C], pos_emb [pos_rows * C], x k-tiled, stats [4 B] or None, C, vocab, pos_rows, absolute_pos)
    table   dict(qkv0 [vocab * 3 C], qkv [B * 3 C], pages (one layer, fp32 or fp16), n_pages, n_head, head_dim, page_table int32
            [B, max_pages], arith_batch=0)
    presence int32 words [B * ceil(V / 32)] (kind 2 with V; kind 4: V = the embedding's vocab)
    scores  kind 2: dict(logprob_step, choice_step [B], logprob_hist, choice_hist [B * stride], stride); kind 4: dict(logprob_hist,
            choice_hist or None, stride, forced=None, forced_stride=0)
    sampler dict(logits [B * V]); rows' logit_bias / min_new_tokens apply (the BIAS form) when any row sets one
    grammar dict(class_of [V], next [n_state * n_class], n_state, n_class, states [B])
    The buffers' sizes and the indices the kernels follow unguarded (ctx_len, row_step >= 0, page table entries) are checked here;
    what the native call refuses raises RuntimeError and launches nothing."""
    from .decoder import pack_row_logits, pack_rows
    lib = _lib.load()
    a = _lib.StepTailArgs()
    keep = []
    i32, f32 = torch.int32, torch.float32
    a.kind, a.B, a.n_steps, a.eos_id = int(kind), int(B), int(state["n_steps"]), int(eos_id)
    nb = max(int(B), 0)
    for k in ("cur_ids", "ctx_len", "done", "row_step"):
        t = _buf(state.get(k), nb, i32, f"step_tail: {k}")
        setattr(a, k + "_dev", None if t is None else t.data_ptr())
        if t is not None and k in ("ctx_len", "row_step") and nb and int(t[:nb].min()) < 0:
            raise RuntimeError(f"step_tail: {k} must not be negative")
    a.n_done_dev = ptr(_buf(state.get("n_done"), 1, i32, "step_tail: n_done"))
    a.ids_out_dev = ptr(_buf(state.get("ids_out"), nb * a.n_steps, i32, "step_tail: ids_out"))
    vocab = int(embed["vocab"]) if embed else 0
    if rows is not None:
        rows = list(rows)
        if len(rows) != nb:
            raise RuntimeError(f"step_tail: {nb} rows but {len(rows)} records")
        recs = pack_rows(rows, vocab if kind == _lib.TAIL_SAMPLE else 14336)
        keep.append(recs)
        a.rows = recs
        if kind == _lib.TAIL_SAMPLE:
            lrecs, kp = pack_row_logits(rows, vocab, state["cur_ids"].device)
            keep += [lrecs, kp]
            if lrecs is not None:
                a.logits_rows = lrecs
    if ctx_cap is not None:
        caps = (C.c_int32 * nb)(*[int(c) for c in ctx_cap])
        keep.append(caps)
        a.ctx_cap = caps
    if partials is not None:
        pval, pidx, n_tiles = partials
        a.n_tiles = int(n_tiles)
        a.pval_dev = ptr(_buf(pval, nb * a.n_tiles, f32, "step_tail: pval"))
        a.pidx_dev = ptr(_buf(pidx, nb * a.n_tiles, i32, "step_tail: pidx"))
    a.sampled_dev = ptr(_buf(sampled, nb, i32, "step_tail: sampled"))
    if embed is not None:
        Cm, pr = int(embed["C"]), int(embed["pos_rows"])
        a.C, a.vocab, a.pos_rows, a.absolute_pos = Cm, vocab, pr, int(embed.get("absolute_pos", 0))
        a.tok_emb_dev = ptr(_buf(embed["tok_emb"], vocab * Cm, f32, "step_tail: tok_emb"))
        a.pos_emb_dev = ptr(_buf(embed["pos_emb"], pr * Cm, f32, "step_tail: pos_emb"))
        a.x_dev = ptr(_buf(embed["x"], tiled_floats(nb, Cm) if Cm % 32 == 0 or nb <= 64 else 0, f32, "step_tail: x"))   # (else: the native call refuses)
        a.stats_dev = ptr(_buf(embed.get("stats"), 4 * nb, f32, "step_tail: stats"))
    if table is not None:
        if embed is None:
            raise RuntimeError("step_tail: the table form needs the embedding")
        H, dh, n_pages = int(table["n_head"]), int(table["head_dim"]), int(table["n_pages"])
        pages = table["pages"]
        if pages.dtype not in (f32, torch.float16):
            raise RuntimeError("step_tail: pages are fp32 or fp16")
        _buf(pages, kv_page_elems(n_pages, H, dh), pages.dtype, "step_tail: pages")
        pt = table["page_table"]
        if pt.ndim != 2 or pt.shape[0] != nb or _buf(pt, 0, i32, "step_tail: page_table") is None or int(pt.min()) < 0 or int(pt.max()) >= n_pages:
            raise RuntimeError("step_tail: page_table is int32 [B, max_pages] with entries in [0, n_pages)")
        a.qkv0_dev = ptr(_buf(table["qkv0"], vocab * 3 * a.C, f32, "step_tail: qkv0"))
        a.qkv_dev = ptr(_buf(table.get("qkv"), nb * 3 * a.C, f32, "step_tail: qkv"))
        a.pages_dev, a.page_table_dev = ptr(pages), ptr(pt)
        a.n_pages, a.page_dtype = n_pages, (_lib.DTYPE_F16 if pages.dtype == torch.float16 else _lib.DTYPE_F32)
        a.n_head, a.head_dim, a.arith_batch, a.max_pages = H, dh, int(table.get("arith_batch", 0)), int(pt.shape[1])
    a.V = vocab if kind == _lib.TAIL_SAMPLE else int(V)
    a.presence_dev = ptr(_buf(presence, nb * presence_words(a.V), i32, "step_tail: presence"))
    if scores is not None:
        st = int(scores["stride"])
        a.hist_stride = st
        a.logprob_hist_dev = ptr(_buf(scores["logprob_hist"], nb * st, f32, "step_tail: logprob_hist"))
        a.choice_hist_dev = ptr(_buf(scores.get("choice_hist"), nb * st, f32, "step_tail: choice_hist"))
        a.logprob_step_dev = ptr(_buf(scores.get("logprob_step"), nb, f32, "step_tail: logprob_step"))
        a.choice_step_dev = ptr(_buf(scores.get("choice_step"), nb, f32, "step_tail: choice_step"))
        a.forced_stride = int(scores.get("forced_stride", 0))
        a.forced_dev = ptr(_buf(scores.get("forced"), nb * max(a.forced_stride, 1), i32, "step_tail: forced"))
    if sampler is not None:
        a.logits_dev = ptr(_buf(sampler["logits"], nb * a.V, f32, "step_tail: logits"))
    if grammar is not None:
        ns, nc = int(grammar["n_state"]), int(grammar["n_class"])
        cls = _buf(grammar["class_of"], a.V, i32, "step_tail: class_of")
        nxt = _buf(grammar["next"], ns * nc, i32, "step_tail: next")
        sts = _buf(grammar["states"], nb, i32, "step_tail: states")
        if int(cls.min()) < 0 or int(cls.max()) >= nc or int(nxt.max()) >= ns or int(sts.max()) >= ns:
            raise RuntimeError("step_tail: grammar tables out of range")
        a.class_of_dev, a.next_dev, a.states_dev, a.n_state, a.n_class = ptr(cls), ptr(nxt), ptr(sts), ns, nc
    a.err_flag_dev = ptr(_buf(err_flag, 1, i32, "step_tail: err_flag"))
    check(lib.mgea_op_step_tail(C.byref(a), stream_ptr()))
    del keep


def dec_embed(form: int, ids: torch.Tensor, tok_emb: torch.Tensor, pos_emb: torch.Tensor, x_out: torch.Tensor, aux_out=None, *,
              lens=None, ctx_len=None, ln_w=None, ln_b=None, eps: float = 1e-5, absolute_pos: int = 0, err_flag=None) -> None:
    """The fp32 prefill embedding through mgea_op_dec_embed: ids int32 [B, T]; form 0 = embed_stats_kernel (x_out k-tiled, aux_out =
    stats [B T, 4]), form 1 = embed_ln_kernel (x_out [B T, C] row-major, aux_out = xn, written when ln_w is given).  In place."""
    lib = _lib.load()
    B, T = ids.shape
    vocab, Cm = tok_emb.shape
    i32, f32 = torch.int32, torch.float32
    M = B * T
    _buf(ids, M, i32, "dec_embed: ids"), _buf(tok_emb, 0, f32, "dec_embed: tok_emb"), _buf(pos_emb, Cm, f32, "dec_embed: pos_emb")
    _buf(x_out, (tiled_floats(M, Cm) if Cm % 32 == 0 or M <= 64 else 0) if form == 0 else M * Cm, f32, "dec_embed: x_out")
    _buf(aux_out, 4 * M if form == 0 else M * Cm, f32, "dec_embed: aux_out")
    _buf(lens, B, i32, "dec_embed: lens"), _buf(ctx_len, B, i32, "dec_embed: ctx_len")
    if ctx_len is not None and int(ctx_len.min()) < 0:
        raise RuntimeError("dec_embed: ctx_len must not be negative")
    _buf(ln_w, Cm, f32, "dec_embed: ln_w"), _buf(ln_b, Cm, f32, "dec_embed: ln_b"), _buf(err_flag, 1, i32, "dec_embed: err_flag")
    check(lib.mgea_op_dec_embed(int(form), ptr(ids), ptr(lens), ptr(ctx_len), ptr(tok_emb), ptr(pos_emb), ptr(x_out), ptr(aux_out), ptr(ln_w),
                                ptr(ln_b), float(eps), B, T, Cm, vocab, pos_emb.shape[0], int(absolute_pos), ptr(err_flag), stream_ptr()))


def take_last(ids: torch.Tensor, lens: Optional[torch.Tensor], cur_ids: torch.Tensor) -> None:
    """cur_ids[b] = ids[b, n - 1], n = lens[b] (None: T) clamped to [1, T] (mgea_op_take_last); in place"""
    B, T = ids.shape
    _buf(ids, B * T, torch.int32, "take_last: ids"), _buf(lens, B, torch.int32, "take_last: lens"), _buf(cur_ids, B, torch.int32, "take_last: cur_ids")
    check(_lib.load().mgea_op_take_last(ptr(ids), ptr(lens), ptr(cur_ids), B, T, stream_ptr()))


def add_lens(ctx_len: torch.Tensor, lens: Optional[torch.Tensor], T: int, B: int) -> None:
    """ctx_len[b] += lens[b] (None: T) for b < B (mgea_op_add_lens); in place"""
    _buf(ctx_len, B, torch.int32, "add_lens: ctx_len"), _buf(lens, B, torch.int32, "add_lens: lens")
    check(_lib.load().mgea_op_add_lens(ptr(ctx_len), ptr(lens), int(T), int(B), stream_ptr()))


def presence_seed(ids: torch.Tensor, lens: Optional[torch.Tensor], V: int, presence: torch.Tensor) -> None:
    """presence rows [B, ceil(V / 32)] (int32 words) <- the sets of the rows' first lens[b] ids (mgea_op_presence_seed); in place"""
    B, T = ids.shape
    _buf(ids, B * T, torch.int32, "presence_seed: ids"), _buf(lens, B, torch.int32, "presence_seed: lens")
    _buf(presence, B * presence_words(min(max(int(V), 0), 14336)), torch.int32, "presence_seed: presence")
    check(_lib.load().mgea_op_presence_seed(ptr(ids), ptr(lens), B, T, int(V), ptr(presence), stream_ptr()))


def unpark_rows(done: torch.Tensor, ctx_len: torch.Tensor, B: int) -> None:
    """done 2 -> 1 with ctx_len + 1 for b < B (mgea_op_unpark_rows); in place"""
    _buf(done, B, torch.int32, "unpark_rows: done"), _buf(ctx_len, B, torch.int32, "unpark_rows: ctx_len")
    check(_lib.load().mgea_op_unpark_rows(ptr(done), ptr(ctx_len), int(B), stream_ptr()))


def grammar_allow(nxt: torch.Tensor, allow: torch.Tensor) -> None:
    """allow [n_state, ceil(n_class / 32)] int32 words <- next [n_state, n_class] >= 0 (mgea_op_grammar_allow); in place"""
    ns, nc = nxt.shape
    taken = 1 <= ns <= 4096 and 1 <= nc <= 4096 and ns * nc <= 1 << 20    # (a shape the call refuses needs no room)
    _buf(nxt, ns * nc, torch.int32, "grammar_allow: next"), _buf(allow, ns * ((nc + 31) // 32) if taken else 0, torch.int32, "grammar_allow: allow")
    check(_lib.load().mgea_op_grammar_allow(ptr(nxt), ns, nc, ptr(allow), stream_ptr()))


def row_budgets(B: int, T: int, *, config=None, rows=None, lens: Optional[torch.Tensor] = None, reserved: int = 0):
    """The rows' device records as a generation builds them (mgea_op_row_budgets), read back as a list of dicts (temperature, top_k,
    top_p, penalty, eos_id, max_new, seed, stream, ctx_cap).  config = dict(temperature, top_k, top_p, eos_id, seed): the uniform
    form, stream = b; or rows = B mgea.decoder.RowSampling.  reserved > 0: the budgets are clamped to the reservation."""
    from .decoder import pack_rows
    s = None if config is None else C.byref(SamplerConfig(**config))
    recs = None if rows is None else pack_rows(list(rows), 14336)
    _buf(lens, B, torch.int32, "row_budgets: lens")
    out, caps = (_lib.RowSampler * B)(), (C.c_int32 * B)()
    check(_lib.load().mgea_op_row_budgets(s, recs, int(B), ptr(lens), int(T), int(reserved), out, caps, stream_ptr()))
    return [dict(temperature=r.temperature, top_k=r.top_k, top_p=r.top_p, penalty=r.repetition_penalty, eos_id=r.eos_id,
                 max_new=r.max_new_tokens, seed=r.seed, stream=r.stream, ctx_cap=int(c)) for r, c in zip(out, caps)]
