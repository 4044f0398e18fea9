"""Host side of the decode-GEMM tests (tests/test_gpu_decode_gemm.py, checked by tests/test_decode_gemm_host.py): the exact-integer
operands, the shapes they are used at, the fp64 references and the expected KV page image.  CPU torch only.

EXACT OPERANDS.  A[m,k] = ((29 m + 13 k) mod 7) - 3 and W[n,k] = ((131 n + 71 k) mod 17) - 8 with integer bias and residual: every
product is an integer of magnitude <= 24, every partial sum over K <= 4096 terms an integer below 2^24 (|sum| <= 98 304 + bias +
residual), so an fp32 evaluation is exact in ANY summation order and the kernels must return the int64 product bit for bit.  Every
operand is at most 8 in magnitude, hence exact in fp16 too: the fp16-weight kernels get the same answer.  The operands depend on m, n
and k individually (7, 17 and the multipliers are pairwise coprime), so a permutation applied to one operand only cannot cancel."""
import math

import numpy as np
import torch

EPI_QKV, EPI_RES, EPI_ACT, EPI_LOGITS = 0, 1, 2, 3
DG_SKINNY, DG_HEAD, DG_GEMV = 0, 1, 2
LIFT = 1 << 20          # added to the bias of the duplicated head rows: above every |sum|, the total still below 2^24

# every (M, N, K) the GPU tests run with the integer operands (the host test proves the premise for each)
GEMV_RES = [(512, 512), (512, 2048), (256, 1280), (1024, 4096), (2048, 256)]
GEMV_ACT = [(512, 2048), (3072, 768)]
GEMV_LOGITS = [(8324, 512), (300, 256), (17, 1280), (5, 512)]
F16_SHAPES = [(64, 512, 512), (5, 512, 2048), (33, 1024, 768), (200, 512, 2048)]
F16_LOGITS = [(64, 8324, 512), (3, 8324, 512), (48, 8324, 1024)]
FEW_WAVE_K = {96: 3, 160: 5, 288: 3, 352: 1, 704: 2}          # K -> waves per workgroup (csrc/gemm_skinny.hip pick_waves)
# M = 200, N = 512 lowers to 16-row tiles (fewer than 256 workgroups otherwise): one epilogue pass.  N = 1024 keeps the 64-row tile, whose
# 256 epilogue items need more than one pass of 64 * nw threads at nw <= 3.
FEW_WAVE_MN = [(200, 512), (16, 512), (200, 1024)]
FEW_WAVE_LOGITS = (48, 4100)

# tests/test_gpu_gemm16_plan.py: the 16-bit GEMM families (bf16 / fp16 operands AND outputs) on the same operands
GEMM16_SHAPES = [(128, 128, 64), (512, 256, 64), (1000, 512, 128), (8192, 4096, 64), (2048, 256, 64)]


def exact_shapes():
    s = [(m, n, k) for m in (1, 2) for n, k in GEMV_RES + GEMV_ACT + GEMV_LOGITS]
    s += F16_SHAPES + F16_LOGITS
    s += [(m, n, k) for k in FEW_WAVE_K for m, n in FEW_WAVE_MN + [FEW_WAVE_LOGITS]]
    return s


def int_a(M, K):
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    return (29 * m + 13 * k) % 7 - 3


def int_w(N, K):
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return (131 * n + 71 * k) % 17 - 8


def int_bias(N):
    return (37 * torch.arange(N)) % 23 - 11


def int_res(M, N):
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return (5 * m + 3 * n) % 19 - 9


def int_product(a, w, bias=None, res=None):
    """a @ w^T (+ bias) (+ res) as int64.  (fp64 matmul of integers below 2^53 is exact and runs on BLAS.)"""
    out = (a.double() @ w.double().t()).long()
    assert bool((out.double() == a.double() @ w.double().t()).all())
    if bias is not None:
        out = out + bias.long()
    if res is not None:
        out = out + res.long()
    return out


def pick_waves(K):
    """csrc/gemm_skinny.hip pick_waves: the most waves <= 8 that divide the 32-wide k-chunks evenly"""
    return next(nw for nw in range(8, 0, -1) if (K // 32) % nw == 0)


def fp32_sum_orders(a, w):
    """a [M, K] @ w [N, K]^T evaluated in fp32, one addition at a time, in three orders: k ascending, k descending, and the skinny
    kernel's split (wave i of pick_waves(K) sums its K / nw slice in order, the partials are added in wave order) -> three [M, N] fp32"""
    a32, w32 = a.float(), w.float()
    K = a.shape[1]

    def run(ks):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
        for k in ks:
            acc = acc + a32[:, k, None] * w32[None, :, k]
        return acc
    nw = pick_waves(K) if K % 32 == 0 else 1
    kw = K // nw
    parts = [run(range(i * kw, (i + 1) * kw)) for i in range(nw)]
    split = parts[0]
    for p in parts[1:]:
        split = split + p
    return run(range(K)), run(range(K - 1, -1, -1)), split


def head_dups(N):
    """the three duplicated head rows (ties across waves and workgroups); a vocabulary of 5 has no row 5"""
    return [5, N // 2 + 3, N - 1] if N > 8 else [0, N // 2, N - 1]


def first_argmax(x):
    """lowest index of each row's maximum"""
    return [int((r == r.max()).nonzero()[0]) for r in x]


# ---- fp64 references -------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def ln_operands(M, N, K, seed):
    """the operand distribution of tests/test_gpu_ops.py test_skinny_gemm_ln_gelu: x = U(-1, 1) + 0.3, W = U(-1, 1) K^-0.5"""
    x = rnd(M, K, seed=seed) + 0.3
    w = rnd(N, K, seed=seed + 1, scale=K ** -0.5)
    b, g, be = rnd(N, seed=seed + 2), 1 + 0.1 * rnd(K, seed=seed + 3), 0.1 * rnd(K, seed=seed + 4)
    return x, w, b, g, be


def tile_stats(x):
    """(mean, M2) of every 16-column tile of x [M, K] -> [M, K/16, 2] (what a residual epilogue leaves)"""
    t = x.double().reshape(x.shape[0], -1, 16)
    mean = t.mean(-1)
    return torch.stack([mean, ((t - mean[..., None]) ** 2).sum(-1)], -1).float()


def row_stats64(x, eps=1e-5):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps)


def ln_gemm64(x, w, b, g, be, eps=1e-5):
    """LN(x) W^T + b in fp64"""
    mean, rstd = row_stats64(x, eps)
    return ((x.double() - mean) * rstd * g.double() + be.double()) @ w.double().t() + b.double()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def f16_model64(x, w, b, g, be, eps=1e-5):
    """The fp16-weight kernels' documented model (csrc/gemm_skinny.hip), every sum in fp64:
        rstd (sum_k half(float(gamma_k x_k)) half(W_nk) - mean c1_n) + c2_n,  c1 = sum_k gamma_k half(W_nk),  c2 = sum_k beta_k half(W_nk) + b_n
    with mean and rstd of x in fp64.  The two roundings are the kernel's: the fp32 product gamma x rounded to fp16, W rounded to fp16."""
    xg = (g.float()[None, :] * x.float()).half().double()
    wh = w.float().half().double()
    mean, rstd = row_stats64(x, eps)
    c1 = wh @ g.double()
    c2 = wh @ be.double() + b.double()
    return rstd * (xg @ wh.t() - mean * c1[None, :]) + c2[None, :]


def f16_model_slow(x, w, b, g, be, m, n, eps=1e-5):
    """one element of f16_model64 by scalar arithmetic (numpy fp32 / fp16 conversions, math.fsum): the independent evaluation"""
    xs = [float(v) for v in x[m].tolist()]
    K = len(xs)
    mean = math.fsum(xs) / K
    var = math.fsum((v - mean) ** 2 for v in xs) / K
    rstd = 1.0 / math.sqrt(var + eps)
    acc, c1, c2 = [], [], []
    for k in range(K):
        wh = float(np.float16(np.float32(w[n, k].item())))
        xg = float(np.float16(np.float32(g[k].item()) * np.float32(x[m, k].item())))
        acc.append(xg * wh)
        c1.append(float(g[k]) * wh)
        c2.append(float(be[k]) * wh)
    return rstd * (math.fsum(acc) - mean * math.fsum(c1)) + math.fsum(c2) + float(b[n])


# ---- the expected KV page image ---------------------------------------------------------------------------------------------
def expected_image(ops, qkv_out, n_head, head_dim, page_table, ctx_len, lens, T, n_pages, layer, n_layers, dtype):
    """What a QKV epilogue must leave in an image of n_layers layers of n_pages pages that started as poison: K | V of the launch's
    own qkv_out [B * T, 3 C] (rounded once with .half() for fp16 pages) at position ctx_len[b] + t of layer `layer` for t < lens[b]
    (lens None: every t), nothing for positions in logical pages >= page_table.shape[1], and poison everywhere else."""
    C = n_head * head_dim
    B = qkv_out.shape[0] // T
    per_layer = ops.kv_page_elems(n_pages, n_head, head_dim)
    img = ops.poison(n_layers * per_layer, dtype)
    kv = qkv_out.cpu().float()[:, C:].to(dtype)
    k = kv[:, :C].reshape(B, T, n_head, head_dim)
    v = kv[:, C:].reshape(B, T, n_head, head_dim)
    valid = None if lens is None else (np.arange(T)[None, :] < np.asarray(lens)[:, None])
    ops.kv_pages_write(img[layer * per_layer:(layer + 1) * per_layer], k, v, np.asarray(page_table), pos0=[int(c) for c in ctx_len], valid=valid)
    return img


def int_bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def permuted_table(B, max_pages, n_pages, mult=7, add=3):
    """[B, max_pages] distinct physical pages that are not the identity: logical (b, j) -> (mult (b max_pages + j) + add) mod n_pages"""
    assert math.gcd(mult, n_pages) == 1 and n_pages >= B * max_pages
    t = (mult * np.arange(B * max_pages) + add) % n_pages
    assert len(set(t.tolist())) == B * max_pages and (t != np.arange(B * max_pages)).any()
    return t.reshape(B, max_pages).astype(np.int32)
