"""The decode-step GEMMs one kernel family, instantiation and epilogue at a time, through mgea_op_decode_gemm (test-only entry: any
plan of plan_decode_gemm on caller buffers, and what ran comes back in plan_out).

EXACT cases (no LayerNorm, no GELU): the integer operands of tests/decode_gemm_util.py make every fp32 partial sum an integer below
2^24, so the int64 product is the answer in any summation order and the assertion is torch.equal.  A dropped or doubled k-chunk, a
fragment read from the wrong (n, k) or a column owned by the wrong lane moves an element by at least 1.
LayerNorm / GELU cases in fp32 are held to fp64 at the project's 2e-5 (tests/test_gpu_ops.py, same operand distribution).
KV page images start as a poison bit pattern on both sides; the expected image is built on the host from the launch's own qkv_out
(whose values are held to fp64) and must equal the device image bit for bit: every written element, every untouched one, the other
layer, and the row whose position lies past the page table.
fp16-weight LayerNorm cases are held to the kernels' documented model evaluated in fp64 (decode_gemm_util.f16_model64): F16_LN_BOUND.

Mutations each exact family was shown to catch (made in a scratch copy, never committed) are listed in DESIGN.md."""
import numpy as np
import pytest
import torch

import decode_gemm_util as U
from decode_gemm_util import DG_GEMV, DG_HEAD, DG_SKINNY, EPI_ACT, EPI_LOGITS, EPI_QKV, EPI_RES

pytestmark = pytest.mark.gpu

TOL, STATS_TOL = 2e-5, 1e-4          # tests/test_gpu_ops.py: fp32 GEMM / LayerNorm / GELU against fp64; tile statistics
MAX_PAGES = 3
# fp16-weight LayerNorm cases: max |kernel - fp64 model| measured on MI355X over M in {3, 37, 64}, ACT (N = 1024, GELU) and QKV (N = 3 K):
#   K = 256: 6.4e-7   K = 512: 4.9e-7   K = 768: 5.0e-7   K = 1024: 6.5e-7
# The bound is twice the measured maximum rounded up to one significant digit (fp32 summation noise moves by about that much between
# shapes and seeds).
F16_LN_BOUND = {256: 2e-6, 512: 1e-6, 768: 1e-6, 1024: 2e-6}


@pytest.fixture(scope="module")
def ops():
    from mgea import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


def refused(ops, *args, **kw):
    """the call must be refused with MGEA_EINVAL (RuntimeError itself, not the MgeaError of a HIP failure)"""
    with pytest.raises(RuntimeError) as e:
        ops.decode_gemm(*args, **kw)
    assert type(e.value) is RuntimeError and not str(e.value).startswith("decode_gemm:"), e.value   # the library's refusal, not the wrapper's
    torch.cuda.synchronize()


def tiled_with_poison_rows(ops, rows, N):
    """k-tiled buffer of one 64-row group: `rows` [M, N] on top, the poison bit pattern in rows >= M"""
    full = ops.poison(64 * N).view(64, N).clone()
    full[: rows.shape[0]] = rows
    return ops.tile_rows(full.cuda())


def check_tiled_rows(ops, buf, want, N):
    """rows < M of the k-tiled buffer equal `want` bit for bit, rows >= M still hold the poison"""
    M = want.shape[0]
    got = ops.untile_rows(buf, 64, N).cpu()
    assert torch.equal(got[:M], want), f"max |diff| {float((got[:M].double() - want.double()).abs().max())}"
    assert bool((U.int_bits(got[M:]) == ops.POISON_BITS).all()), "rows >= M of the tiled buffer were written"


def check_partials(ops, extras, plan, M, logits):
    """the LOGITS partials fill exactly the documented layout and merge to the first index of each row's maximum"""
    R, P = extras["R"], extras["P"]
    assert P == plan["n_partials"] > 0
    bits = U.int_bits(extras["partials"].cpu())
    val, idx = bits[: R * P].view(R, P), bits[R * P: 2 * R * P].view(R, P)
    assert not bool((val[:M] == ops.POISON_BITS).any()) and not bool((idx[:M] == ops.POISON_BITS).any()), "a partial of a live row was not written"
    assert bool((val[M:] == ops.POISON_BITS).all()) and bool((idx[M:] == ops.POISON_BITS).all()), "rows >= M were written"
    assert bool((bits[2 * R * P:] == ops.POISON_BITS).all()), "the partials overran their layout"
    assert ops.merge_partials(extras["partials"], M, R, P).tolist() == U.first_argmax(logits)


def run_exact_logits(ops, M, N, K, wdev, plan_check, **kw):
    """LOGITS with the integer operands: exact logits, partials layout, ties across waves and workgroups, out = NULL"""
    a, w, b = U.int_a(M, K), U.int_w(N, K), U.int_bias(N)
    hi = U.head_dups(N)
    w[hi[1]] = w[hi[0]]; w[hi[2]] = w[hi[0]]
    b[hi[1]] = b[hi[0]]; b[hi[2]] = b[hi[0]]
    at, wd = ops.tile_rows(a.float().cuda()), wdev(w.float().cuda())
    want = U.int_product(a, w, b).float()
    out, ex, plan = ops.decode_gemm(EPI_LOGITS, at, wd, b.float().cuda(), M, N, K, **kw)
    plan_check(plan)
    assert torch.equal(out.cpu(), want), f"max |diff| {float((out.cpu().double() - want.double()).abs().max())}"
    check_partials(ops, ex, plan, M, want)
    b2 = b.clone()
    b2[hi] += U.LIFT
    want2 = U.int_product(a, w, b2).float()
    for want_out in (True, False):
        out, ex, plan = ops.decode_gemm(EPI_LOGITS, at, wd, b2.float().cuda(), M, N, K, want_out=want_out, **kw)
        assert (out is None) == (not want_out)
        if want_out:
            assert torch.equal(out.cpu(), want2)
        check_partials(ops, ex, plan, M, want2)
        assert ops.merge_partials(ex["partials"], M, ex["R"], ex["P"]).tolist() == [hi[0]] * M


# =================================================================================================================================
# (a) gemv_rows_kernel: rowmajor = 1, M in {1, 2}
# =================================================================================================================================
def gemv_plan(plan, M, cw):
    assert plan["kind"] == DG_GEMV and plan["mr"] == M and plan["cw"] == cw, plan


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", U.GEMV_RES)
def test_gemv_residual_exact(ops, M, N, K):
    """<RES, no LN, cw 1 / 2 (N = 2048), mr M>: K of 1, 2, 5 (one full group of 4 steps plus one), 8 and 16 steps; the result lands
    in place in the k-tiled x, rows >= M untouched."""
    a, w, b, res = U.int_a(M, K), U.int_w(N, K), U.int_bias(N), U.int_res(M, N)
    x = tiled_with_poison_rows(ops, res.float(), N)
    out, _, plan = ops.decode_gemm(EPI_RES, ops.tile_rows(a.float().cuda()), w.float().cuda(), b.float().cuda(), M, N, K, rowmajor=True, out=x)
    gemv_plan(plan, M, 2 if N >= 2048 else 1)
    assert plan["grid_x"] == N // (4 * plan["cw"])
    check_tiled_rows(ops, out, U.int_product(a, w, b, res).float(), N)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", U.GEMV_ACT)
@pytest.mark.parametrize("act", [0, 2])
def test_gemv_activation_exact(ops, M, N, K, act):
    """<ACT, no LN, cw 1 / 2 (N = 3072), mr M> with no activation and ReLU"""
    a, w, b = U.int_a(M, K), U.int_w(N, K), U.int_bias(N)
    buf = tiled_with_poison_rows(ops, torch.zeros(M, N), N)
    out, _, plan = ops.decode_gemm(EPI_ACT, ops.tile_rows(a.float().cuda()), w.float().cuda(), b.float().cuda(), M, N, K, rowmajor=True,
                                   act=act, out=buf)
    gemv_plan(plan, M, 2 if N >= 2048 else 1)
    want = U.int_product(a, w, b).float()
    check_tiled_rows(ops, out, want.clamp_min(0) if act == 2 else want, N)
    assert act != 2 or bool((want < 0).any())


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("K", [256, 512, 768, 1024])
def test_gemv_direct_layernorm_activation(ops, M, K):
    """<ACT, LN, cw 1 (N = 1024) / 2 (N = 2048), mr M>: the LayerNorm prologue with 1, 2, 3 and 4 of its KSX = 4 steps live"""
    for N in (1024, 2048):
        x, w, b, g, be = U.ln_operands(M, N, K, seed=100 + K)
        pre = U.ln_gemm64(x, w, b, g, be)
        for act in (1, 0):
            out, _, plan = ops.decode_gemm(EPI_ACT, ops.tile_rows(x.cuda()), w.cuda(), b.cuda(), M, N, K, rowmajor=True, act=act,
                                           ln_g=g.cuda(), ln_b=be.cuda())
            gemv_plan(plan, M, 2 if N >= 2048 else 1)
            err = float((ops.untile_rows(out, M, N).cpu().double() - (U.gelu64(pre) if act else pre)).abs().max())
            print(f"gemv LN-ACT M={M} N={N} K={K} act={act}: max |diff| vs fp64 {err:.3e}")
            assert err < TOL, err


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("C,dh", [(256, 32), (512, 64), (768, 96), (1024, 64)])
def test_gemv_qkv_direct_layernorm_and_page_scatter(ops, M, C, dh):
    """<QKV, LN, cw 1 / 2 (C >= 768), mr M> on fp32 pages: qkv_out against fp64, and the gemv's own KV append against the host image:
    positions 0, 63, 64, 127 and 64 * max_pages (past the table: nothing written), the two rows at different positions, a permuted
    page table, both layers of a two-layer image."""
    H, N, K = C // dh, 3 * C, C
    n_pages = M * MAX_PAGES + 2
    table = U.permuted_table(M, MAX_PAGES, n_pages, mult=3, add=1)
    x, w, b, g, be = U.ln_operands(M, N, K, seed=200 + C)
    want = U.ln_gemm64(x, w, b, g, be)
    at, wd, bd, gd, bed = ops.tile_rows(x.cuda()), w.cuda(), b.cuda(), g.cuda(), be.cuda()
    past = 64 * MAX_PAGES
    ctxs = [[0], [63], [64], [127], [past]] if M == 1 else [[0, 63], [64, 127], [past, 0], [127, past], [63, 64]]
    for i, ctx in enumerate(ctxs):
        for layer in (0, 1):
            pages = ops.poison(2 * ops.kv_page_elems(n_pages, H, dh), device="cuda")
            kv = dict(pages=pages, n_pages=n_pages, n_head=H, head_dim=dh, layer=layer, page_table=torch.from_numpy(table).cuda(),
                      ctx_len=torch.tensor(ctx).cuda())
            out, _, plan = ops.decode_gemm(EPI_QKV, at, wd, bd, M, N, K, rowmajor=True, ln_g=gd, ln_b=bed, kv=kv)
            gemv_plan(plan, M, 2 if N >= 2048 else 1)
            err = float((out.cpu().double() - want).abs().max())
            if i == 0 and layer == 0:
                print(f"gemv LN-QKV M={M} C={C}: max |diff| vs fp64 {err:.3e}")
            assert err < TOL, err
            exp = U.expected_image(ops, out, H, dh, table, ctx, None, 1, n_pages, layer, 2, torch.float32)
            assert torch.equal(U.int_bits(pages.cpu()), U.int_bits(exp)), (ctx, layer)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", U.GEMV_LOGITS)
def test_gemv_logits_exact_and_partials(ops, M, N, K):
    """<LOGITS, cw 4, mr M>: a ragged last workgroup (N = 8324, 300, 17 and 5 are no multiples of 16), one partial per workgroup"""
    def plan_check(plan):
        gemv_plan(plan, M, 4)
        assert plan["grid_x"] == plan["n_partials"] == (N + 15) // 16
    run_exact_logits(ops, M, N, K, lambda w: w, plan_check, rowmajor=True)


def test_gemv_refusals_launch_nothing(ops):
    """Shapes and combinations the dot-product family does not take: MGEA_EINVAL, every output still NaN"""
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    ones = lambda *s: torch.ones(*s, device="cuda")

    def res_case(M, N, K, **kw):
        out = nan((M + 63) // 64 * 64 * N)
        refused(ops, EPI_RES, ones((M + 63) // 64 * 64 * K), ones(N, K), ones(N), M, N, K, rowmajor=True, out=out, **kw)
        assert bool(out.isnan().all())
    res_case(3, 512, 512)              # M = 3
    res_case(2, 512, 384)              # K no multiple of 256
    res_case(2, 516, 512)              # N no multiple of 8
    out = nan(64 * 512)
    refused(ops, EPI_ACT, ones(64 * 2048), ones(512, 2048), ones(512), 2, 512, 2048, rowmajor=True, out=out, ln_g=ones(2048), ln_b=ones(2048))
    assert bool(out.isnan().all())     # LayerNorm prologue with K = 2048
    out = nan(64 * 512)
    refused(ops, EPI_ACT, ones(64 * 512), torch.ones(512 * 512, device="cuda", dtype=torch.float16), ones(512), 2, 512, 512, rowmajor=True,
            w_f16=True, out=out)
    assert bool(out.isnan().all())     # fp16 weights
    H, dh, C = 4, 64, 256
    pages = ops.poison(ops.kv_page_elems(4, H, dh), torch.float16, device="cuda")
    kv = dict(pages=pages, n_pages=4, n_head=H, head_dim=dh, layer=0, page_table=torch.tensor([[1, 0]]).cuda(), ctx_len=torch.tensor([3]).cuda())
    out = nan(1, 3 * C)
    refused(ops, EPI_QKV, ones(64 * C), ones(3 * C, C), ones(3 * C), 1, 3 * C, C, rowmajor=True, ln_g=ones(C), ln_b=ones(C), kv=kv, out=out)
    assert bool(out.isnan().all()) and bool(pages.isnan().all())     # QKV with an fp16 pool


# =================================================================================================================================
# (b) EPI_QKV of gemm_skinny_kernel: rowmajor = 0, LayerNorm folded by ops.fold_ln
# =================================================================================================================================
def run_skinny_qkv(ops, B, T, C, dh, ctx, lens, page_dtype, layer, w_f16=False, bound=TOL, label=""):
    """One QKV launch of the tiled family: qkv_out of the real rows against the reference, zero rows for padded tokens, the device
    page image bit-equal to the host image built from the launch's own K | V.  Returns (plan, max |diff|)."""
    H, N, K, M = C // dh, 3 * C, C, B * T
    n_pages = B * MAX_PAGES + 1
    table = U.permuted_table(B, MAX_PAGES, n_pages, mult=5 if n_pages % 5 else 7, add=2)
    x, w, b, g, be = U.ln_operands(M, N, K, seed=300 + C + M)
    stats = U.tile_stats(x).cuda()
    if w_f16:
        wd = ops.tile_weights_f16(w.cuda())
        c1, c2 = ops.ln_vectors(w.half().float().cuda(), g.cuda(), be.cuda(), b.cuda())
        want = U.f16_model64(x, w, b, g, be)
        extra = dict(w_f16=True, ln_g=g.cuda())
    else:
        wd, c1, c2 = ops.fold_ln(w.cuda(), g.cuda(), be.cuda(), b.cuda())
        want = U.ln_gemm64(x, w, b, g, be)
        extra = {}
    pages = ops.poison(2 * ops.kv_page_elems(n_pages, H, dh), page_dtype, device="cuda")
    kv = dict(pages=pages, n_pages=n_pages, n_head=H, head_dim=dh, layer=layer, page_table=torch.from_numpy(table).cuda(),
              ctx_len=torch.tensor(ctx).cuda(), lens=None if lens is None else torch.tensor(lens).cuda(), T=T)
    out, _, plan = ops.decode_gemm(EPI_QKV, ops.tile_rows(x.cuda()), wd, c2, M, N, K, ln_c1=c1, stats_in=stats, kv=kv, **extra)
    assert plan["kind"] == DG_SKINNY and plan["nt"] == 1, plan
    got = out.cpu()
    real = torch.ones(B, T, dtype=torch.bool) if lens is None else torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    real = real.reshape(-1)
    err = float((got[real].double() - want[real]).abs().max())
    print(f"skinny QKV {label} B={B} T={T} C={C} pages={page_dtype} plan={plan}: max |diff| {err:.3e}")
    assert err < bound, err
    assert bool((got[~real] == 0).all()), "a padded token's qkv_out row is not zero"
    exp = U.expected_image(ops, out, H, dh, table, ctx, lens, T, n_pages, layer, 2, page_dtype)
    assert torch.equal(U.int_bits(pages.cpu()), U.int_bits(exp)), "device page image differs from the host image"
    return plan, err


def decode_ctx(M):
    """0, 1, 62, 63, 64, 65, 127, 128 in turn, and one row past the page table"""
    ctx = [[0, 1, 62, 63, 64, 65, 127, 128][i % 8] for i in range(M)]
    ctx[M // 2] = 64 * MAX_PAGES
    return ctx


@pytest.mark.parametrize("page_dtype", [torch.float32, torch.float16], ids=["f32pages", "f16pages"])
@pytest.mark.parametrize("M,C,dh,mt,nch", [(3, 512, 64, 1, 2), (16, 512, 64, 1, 2), (37, 512, 64, 2, 2), (64, 512, 64, 2, 2), (100, 512, 64, 2, 2),
                                           (37, 256, 32, 1, 0), (37, 768, 96, 2, 3)])
def test_skinny_qkv_decode_step(ops, M, C, dh, mt, nch, page_dtype):
    """T = 1: one new token per row; 16- and 32-row tiles, two 64-row groups (M = 100), the compile-time streams nch 2 and 3 and the
    generic stream (C = 256: 8 waves of one chunk), fp32 and fp16 pages (kv_store4's two layouts)."""
    plan, _ = run_skinny_qkv(ops, M, 1, C, dh, decode_ctx(M), None, page_dtype, layer=M % 2)
    assert (plan["mt"], plan["nw"], plan["nch"]) == (mt, 8, nch), plan


@pytest.mark.parametrize("page_dtype", [torch.float32, torch.float16], ids=["f32pages", "f16pages"])
@pytest.mark.parametrize("B,T,ctx,lens", [
    (3, 5, [62, 0, 125], [5, 1, 3]),
    (3, 5, [62, 0, 125], None),
    (10, 7, [0, 60, 64, 121, 188, 5, 63, 127, 192, 58], [7, 7, 1, 7, 7, 3, 2, 7, 7, 6]),
    (10, 7, [0, 60, 64, 121, 188, 5, 63, 127, 192, 58], None)], ids=["3x5-ragged", "3x5-full", "10x7-ragged", "10x7-full"])
def test_skinny_qkv_fused_prefill_and_extend(ops, B, T, ctx, lens, page_dtype):
    """T > 1: rows cross a page boundary inside a sequence (62 + 5, 125 + 3, 60 + 7, 121 + 7), run off the end of the table (188 + 7:
    positions 192.. are dropped; 192: all dropped), ragged lengths (padded tokens: zero row, nothing cached) and lens = NULL; 70 rows
    are two row groups, so the reload path of the page lookup runs next to the prefetched one."""
    plan, _ = run_skinny_qkv(ops, B, T, 512, 64, ctx, lens, page_dtype, layer=1)
    assert (plan["nw"], plan["nch"]) == (8, 2) and plan["mt"] == (1 if B * T <= 16 else 2), plan


# =================================================================================================================================
# (c) fp16 weights: w_f16 = 1
# =================================================================================================================================
def skinny_plan(plan, f16_kind=DG_SKINNY):
    assert plan["kind"] == f16_kind, plan


@pytest.mark.parametrize("M,N,K", U.F16_SHAPES)
def test_f16_weights_residual_and_activation_exact(ops, M, N, K):
    """gemm_skinny_kernel<.., F16 = true>: RES (with its tile statistics) and ACT (none, ReLU) on tile_weights_f16 fragments.  The
    statistics are checked on the same operands scaled by powers of two (A / 8, W / 64, bias and residual / 8: still exact, outputs of
    order 1), where the project's absolute 1e-4 means something."""
    a, w, b, res = U.int_a(M, K), U.int_w(N, K), U.int_bias(N), U.int_res(M, N)
    at, w16 = ops.tile_rows(a.float().cuda()), ops.tile_weights_f16(w.float().cuda())
    G = (M + 63) // 64
    for act in (0, 2):
        out, _, plan = ops.decode_gemm(EPI_ACT, at, w16, b.float().cuda(), M, N, K, w_f16=True, act=act)
        skinny_plan(plan)
        want = U.int_product(a, w, b).float()
        assert torch.equal(ops.untile_rows(out, M, N).cpu(), want.clamp_min(0) if act == 2 else want)
    print(f"f16 RES/ACT M={M} N={N} K={K}: plan {plan}")
    x = ops.tile_rows(res.float().cuda())
    out, ex, plan = ops.decode_gemm(EPI_RES, at, w16, b.float().cuda(), M, N, K, w_f16=True, out=x)
    assert torch.equal(ops.untile_rows(out, M, N).cpu(), U.int_product(a, w, b, res).float())
    # scaled: (A / 8) (W / 64)^T + b / 8 + res / 8 = (A W^T + 64 b + 64 res) / 512
    want = (U.int_product(a, w, 64 * b, 64 * res).double() / 512).float()
    x = ops.tile_rows((res.float() / 8).cuda())
    out, ex, plan = ops.decode_gemm(EPI_RES, ops.tile_rows((a.float() / 8).cuda()), ops.tile_weights_f16((w.float() / 64).cuda()),
                                    (b.float() / 8).cuda(), M, N, K, w_f16=True, out=x)
    assert torch.equal(ops.untile_rows(out, M, N).cpu(), want)
    serr = float((ex["stats_out"].cpu() - U.tile_stats(want)).abs().max())
    print(f"f16 RES M={M} N={N} K={K}: tile statistics max |diff| {serr:.3e}")
    assert serr < STATS_TOL, serr


@pytest.mark.parametrize("M,N,K,kind", [(64, 8324, 512, DG_HEAD), (3, 8324, 512, DG_HEAD), (48, 8324, 1024, DG_SKINNY)])
def test_f16_weights_logits_exact(ops, M, N, K, kind):
    """head_balanced_kernel<.., f16 = 1> (3 and 64 rows) and the generic 32 x 32 head on fp16 fragments"""
    def plan_check(plan):
        assert plan["kind"] == kind, plan
        if kind == DG_SKINNY:
            assert (plan["mt"], plan["nt"]) == (2, 2), plan
        else:
            assert plan["nch"] == K // 256 and plan["n_partials"] == plan["grid_x"], plan
    run_exact_logits(ops, M, N, K, ops.tile_weights_f16, plan_check, w_f16=True)


@pytest.mark.parametrize("M", [3, 37, 64])
@pytest.mark.parametrize("K", [256, 512, 768, 1024])
def test_f16_weights_layernorm_against_the_documented_model(ops, M, K):
    """ACT (GELU) and QKV with the LayerNorm of the fp16-weight kernels: gamma on the activation side, c1 / c2 from ops.ln_vectors.
    Reference: decode_gemm_util.f16_model64 (fp64 sums of the kernel's own two roundings); only fp32 accumulation separates them.
    Measured on MI355X, max |kernel - model| over M in {3, 37, 64} and both epilogues: K = 256 6.4e-7, K = 512 4.9e-7, K = 768 5.0e-7,
    K = 1024 6.5e-7; the bound is twice that, rounded up to one digit (F16_LN_BOUND).  Before the generic stream kept its gamma * x
    products in fp32 ahead of the fp16 conversion, [256-64] showed 5.1e-5 and [1024-37] 5.8e-5: single elements rounded once
    (v_fma_mix*_f16) instead of twice.  The distance of the model to the unrounded LayerNorm GEMM in fp64 (6e-4 .. 9e-4: the model's own
    fp16 rounding, not the kernel's error) is printed, not asserted."""
    bound = F16_LN_BOUND[K]
    N = 1024
    x, w, b, g, be = U.ln_operands(M, N, K, seed=400 + K + M)
    w16 = ops.tile_weights_f16(w.cuda())
    c1, c2 = ops.ln_vectors(w.half().float().cuda(), g.cuda(), be.cuda(), b.cuda())
    out, _, plan = ops.decode_gemm(EPI_ACT, ops.tile_rows(x.cuda()), w16, c2, M, N, K, w_f16=True, act=1, ln_c1=c1, ln_g=g.cuda(),
                                   stats_in=U.tile_stats(x).cuda())
    skinny_plan(plan)
    model = U.f16_model64(x, w, b, g, be)
    err = float((ops.untile_rows(out, M, N).cpu().double() - U.gelu64(model)).abs().max())
    away = float((model - U.ln_gemm64(x, w, b, g, be)).abs().max())
    print(f"f16 LN-ACT M={M} K={K} plan={plan}: max |kernel - model| {err:.3e}; model vs unrounded fp64 LayerNorm GEMM {away:.3e}")
    dh = {256: 32, 512: 64, 768: 96, 1024: 64}[K]
    _, qerr = run_skinny_qkv(ops, M, 1, K, dh, decode_ctx(M), None, torch.float16, layer=1, w_f16=True, bound=float("inf"), label="f16 weights")
    print(f"F16_LN_MEASURED K={K} M={M} act={err:.3e} qkv={qerr:.3e}")
    assert bound is not None and max(err, qerr) < bound, (err, qerr, bound)


# =================================================================================================================================
# (d) the generic instruction stream with fewer than 8 waves: rowmajor = 0, fp32 tiles
# =================================================================================================================================
@pytest.mark.parametrize("K,nw", sorted(U.FEW_WAVE_K.items()))
def test_few_waves_residual_and_activation_exact(ops, K, nw):
    """RES and ACT at 3, 5, 3, 1 and 2 waves.  (200, 1024) keeps the 64-row tile: 256 epilogue items on 64 * nw threads, so the
    second pass (bias, residual reloaded) runs at nw <= 3; (200, 512) lowers to 16-row tiles, (16, 512) is a single row tile."""
    passes = set()
    for M, N in U.FEW_WAVE_MN:
        a, w, b, res = U.int_a(M, K), U.int_w(N, K), U.int_bias(N), U.int_res(M, N)
        at, wt = ops.tile_rows(a.float().cuda()), ops.tile_weights(w.float().cuda())
        for act in (0, 2):
            out, _, plan = ops.decode_gemm(EPI_ACT, at, wt, b.float().cuda(), M, N, K, act=act)
            assert (plan["kind"], plan["nw"], plan["nch"], plan["nt"]) == (DG_SKINNY, nw, 0, 1), plan
            want = U.int_product(a, w, b).float()
            assert torch.equal(ops.untile_rows(out, M, N).cpu(), want.clamp_min(0) if act == 2 else want), (M, N, act)
        out, _, plan2 = ops.decode_gemm(EPI_RES, at, wt, b.float().cuda(), M, N, K, out=ops.tile_rows(res.float().cuda()))
        assert plan2 == plan
        assert torch.equal(ops.untile_rows(out, M, N).cpu(), U.int_product(a, w, b, res).float()), (M, N)
        assert plan["mt"] == {(200, 512): 1, (16, 512): 1, (200, 1024): 4}[(M, N)], plan
        passes.add(-(-16 * plan["mt"] * 4 // (64 * nw)))
    assert (max(passes) > 1) == (nw <= 3), passes


@pytest.mark.parametrize("K,nw", sorted(U.FEW_WAVE_K.items()))
def test_few_waves_logits_exact(ops, K, nw):
    """the 32 x 32 head tile (mt = nt = 2: 256 epilogue items) at fewer than 8 waves: more than one epilogue pass at nw <= 3"""
    M, N = U.FEW_WAVE_LOGITS

    def plan_check(plan):
        assert (plan["kind"], plan["mt"], plan["nt"], plan["nw"], plan["nch"]) == (DG_SKINNY, 2, 2, nw, 0), plan
    run_exact_logits(ops, M, N, K, ops.tile_weights, plan_check)


@pytest.mark.parametrize("K,nw", sorted(U.FEW_WAVE_K.items()))
def test_few_waves_layernorm_activation_or_refusal(ops, K, nw):
    """LN-ACT at M = 37, N = 1536: the LayerNorm merge wants 16 lanes per tile row, i.e. at least 4 waves for a 16-row tile: only
    K = 160 (5 waves) runs, lowered to 16-row tiles; 1, 2 and 3 waves are refused with MGEA_EINVAL and nothing is launched."""
    M, N = 37, 1536
    x, w, b, g, be = U.ln_operands(M, N, K, seed=500 + K)
    wt, c1, c2 = ops.fold_ln(w.cuda(), g.cuda(), be.cuda(), b.cuda())
    args = (EPI_ACT, ops.tile_rows(x.cuda()), wt, c2, M, N, K)
    kw = dict(act=1, ln_c1=c1, stats_in=U.tile_stats(x).cuda())
    if nw * 64 < 256:
        out = torch.full((64 * N,), float("nan"), device="cuda")
        refused(ops, *args, out=out, **kw)
        assert bool(out.isnan().all())
        return
    out, _, plan = ops.decode_gemm(*args, **kw)
    assert (plan["kind"], plan["mt"], plan["nw"], plan["nch"]) == (DG_SKINNY, 1, nw, 0), plan
    err = float((ops.untile_rows(out, M, N).cpu().double() - U.gelu64(U.ln_gemm64(x, w, b, g, be))).abs().max())
    print(f"few-wave LN-ACT K={K} nw={nw}: max |diff| vs fp64 {err:.3e}")
    assert err < TOL, err
