"""Host side of tests/test_gpu_bert_kernels.py (premises checked on the CPU by tests/test_bert_kernels_host.py): the inputs of the
DistilBERT row kernels and of the split-K slab epilogues, their fp64 references and the bounds.  CPU torch only.

INTEGER SLABS.  P[s][m][n] = ((5 m + 3 n + 7 s) mod 19) - 9 with the integer bias of tests/decode_gemm_util.py: a sum over at most 4
slabs plus bias plus an integer residual stays below 2^7, so every fp32 evaluation is exact in any order, and the values are exact in
fp16 (the KV pages).  The GELU cases use the same numbers times 1/4 (still exact sums): arguments within +-12, where the erf form has
no cancellation to hide behind."""
import math

import numpy as np
import torch

from decode_gemm_util import int_bias, rnd

VOCAB = 50
EMBED_D = {torch.float32: [128, 768, 1028, 2048, 4096], torch.bfloat16: [128, 768, 1028, 2048]}
EMBED_BS = [(3, 7), (1, 1), (2, 64)]
EMBED_PACKED_LENS = (1, 5, 15)
DC_ROW, DC_OFFSET = 7, 50.0                      # the word row that carries a DC offset of +50 against a spread of 1
LN16_C = [8, 128, 520, 768, 1024, 1032, 2048]
LN16_M = [1, 15, 16, 17, 300]
GATHER_SEQS = (1, 5, 15, 2, 64)                  # packed: cu = cumsum
BIAS_ACT_SHAPES = [(1, 28, 28), (5, 301, 301), (3, 1030, 1040), (64, 2048, 2051)]      # (M, N, ldo)
RES_LN_C, RES_LN_M, RES_LN_S = [128, 768, 4096], [1, 5], [1, 4]
LOGITS_V, LOGITS_M, LOGITS_S = [28, 301, 8324], [1, 6], [1, 3]
GEMM_EXACT = [(64, 300, 512), (1, 64, 32), (130, 260, 1024), (7, 311, 128)]
GEMM_SPLITS = [1, 2, 3, 5, 7, 16, 32]
DIRECT_SHAPES = [(65, 128, 32), (300, 260, 96), (1024, 256, 64)]                        # 1, 9 and 16 tiles of 128 x 128
LORA_SHAPES = [(128, 128, 8), (5, 33, 3)]
LIFT = 4096                                      # the duplicated row maximum of the argmax tests: above every natural sum


def bf16_bound(want):
    """|got - want| <= 2^-8 |want| + 2e-5: one correct bf16 rounding (half an ulp is at most 2^-8 of the value) plus the fp32 error that
    can move the value across a rounding boundary (the bound of the fp32 LayerNorm tests)"""
    return 2.0 ** -8 * want.abs() + 2e-5


def ln64(x, w, b, eps):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- embedding -----------------------------------------------------------------------------------------------------------------
def embed_tables(D, max_pos, seed=0):
    """word [VOCAB, D] (row DC_ROW = +50 + a spread of 1), pos [max_pos, D], ln_w, ln_b"""
    word = rnd(VOCAB, D, seed=seed)
    word[DC_ROW] += DC_OFFSET
    return word, rnd(max_pos, D, seed=seed + 1, scale=0.5), 1 + 0.1 * rnd(D, seed=seed + 2), 0.1 * rnd(D, seed=seed + 3)


def embed_ids(B, S, packed, seed=0):
    """-> (ids, pos_ids, t): padded ids [B, S] with t = the column; packed ids [rows] with positions restarting per sequence.  Every
    call holds DC_ROW, the first and the last vocabulary row."""
    g = torch.Generator().manual_seed(100 + seed)
    if packed:
        t = torch.cat([torch.arange(n) for n in EMBED_PACKED_LENS])
        ids = torch.randint(0, VOCAB, (t.numel(),), generator=g)
        ids[0], ids[3], ids[-1] = DC_ROW, 0, VOCAB - 1
        return ids.to(torch.int32), t.to(torch.int32), t.long()
    ids = torch.randint(0, VOCAB, (B, S), generator=g)
    ids.view(-1)[0] = DC_ROW
    if B * S > 2:
        ids.view(-1)[1], ids.view(-1)[-1] = 0, VOCAB - 1
    return ids.to(torch.int32), None, torch.arange(S).repeat(B)


def embed_ref(ids, t, word, pos, ln_w, ln_b, eps):
    """fp64 LayerNorm of word[id] + pos[t] (ids clamped to the vocabulary, as the kernel documents)"""
    idc = ids.reshape(-1).long().clamp(0, VOCAB - 1)
    return ln64(word.double()[idc] + pos.double()[t], ln_w, ln_b, eps)


# ---- gather -------------------------------------------------------------------------------------------------------------------
def gather_inputs(B, S, D, packed, seed=0):
    """h [rows, D] fp32 with |h| <= 4 (NaN in every row that is not a [CLS] row), rowstat [rows, 2] with |mean| <= 0.3 and rstd in
    [0.5, 1.5], gamma in [0.8, 1.2], beta, cu (or None), the [CLS] row of every sequence"""
    if packed:
        assert B == len(GATHER_SEQS)
        cu = torch.tensor(np.concatenate([[0], np.cumsum(GATHER_SEQS)]), dtype=torch.int32)
        first, rows = cu[:-1].long(), int(cu[-1])
    else:
        cu, first, rows = None, torch.arange(B) * S, B * S
    h = torch.full((rows, D), float("nan"))
    h[first] = rnd(B, D, seed=seed, scale=4.0)
    rowstat = torch.full((rows, 2), float("nan"))
    rowstat[first, 0] = rnd(B, seed=seed + 1, scale=0.3)
    rowstat[first, 1] = 1.0 + rnd(B, seed=seed + 2, scale=0.5)
    return h, rowstat, 1 + rnd(D, seed=seed + 3, scale=0.2), rnd(D, seed=seed + 4, scale=0.5), cu, first


# ---- slabs --------------------------------------------------------------------------------------------------------------------
def int_slabs(S, M, ldp, N=None):
    """[S, M, ldp] integers in [-9, 9] that differ between slabs, rows and columns; columns >= N (the slab padding) are NaN"""
    s, m, n = torch.arange(S)[:, None, None], torch.arange(M)[None, :, None], torch.arange(ldp)[None, None, :]
    p = ((5 * m + 3 * n + 7 * s) % 19 - 9).float()
    if N is not None:
        p[:, :, N:] = float("nan")
    return p


def int_x(M, C):
    m, n = torch.arange(M)[:, None], torch.arange(C)[None, :]
    return ((11 * m + 7 * n) % 23 - 11).float()


def slab_sum(P, N, bias=None):
    """the exact answer: sum over the slabs (+ bias) of columns < N, int64"""
    out = P[:, :, :N].long().sum(0)
    return out if bias is None else out + bias[:N].long()


def argmax_slabs(S, M, V, shift):
    """integer slabs [S, M, V] whose row m follows pattern (m + shift) % 3: 0 = the row maximum LIFT duplicated in three columns that
    different waves scan (n, n + 64, n + 256: thread n of wave 0, thread n + 64 of wave 1, thread n again one stride later), as far
    as they exist; 1 = LIFT at a middle column and at the LAST column; 2 = the natural sums (small integers with many ties).
    -> (P, bias, logits int64 [M, V], the first index of each row's maximum)"""
    P, bias = int_slabs(S, M, V), int_bias(V)
    L = slab_sum(P, V, bias)
    for m in range(M):
        kind = (m + shift) % 3
        cols = [c for c in (5 + m, 5 + m + 64, 5 + m + 256) if c < V] if kind == 0 else [V // 2 + 1, V - 1] if kind == 1 else []
        for c in cols:
            P[0, m, c] += float(LIFT - L[m, c])
    L = slab_sum(P, V, bias)
    first = [int((r == r.max()).nonzero()[0]) for r in L]
    return P, bias, L, first


def scatter_case(dh, lens, max_pages, H=2, B=2, T=3, S=3):
    """the qkv epilogue's inputs: slabs [S, B T, 3 C + 8] (padding NaN), bias, ctx_len [62, 130] -> (P, bias, ctx_len, expected qkv_out
    int64 [B T, 3 C] with zero rows past lens)"""
    C = H * dh
    P, bias = int_slabs(S, B * T, 3 * C + 8, 3 * C), int_bias(3 * C)
    want = slab_sum(P, 3 * C, bias)
    if lens is not None:
        real = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
        want = want * real[:, None]
    return P, bias, [62, 130], want


def n_pages_for(B, max_pages):
    return 8 if B * max_pages <= 8 else B * max_pages + 1
