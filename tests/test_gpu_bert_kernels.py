"""The DistilBERT row kernels, the [CLS] gathers and the split-K slab epilogues, one kernel per call on caller buffers (mgea_op_bert_embed,
mgea_op_gather_cls, mgea_op_slab_*, mgea_op_gemm_f32_direct, mgea_lora_merge; the [CLS] attention is in test_gpu_attention_exact.py).

Every output element is checked.  Where the operands are the integers of tests/decode_gemm_util.py / tests/bert_kernels_util.py the
answer is exact in fp32 in ANY summation order and the kernel must return it bit for bit; the LayerNorm / GELU cases are held to an fp64
reference at bounds that come from the project's own fp32 tests (2e-5) or from the number format (bert_kernels_util.bf16_bound), never
from what the kernels gave.  tests/test_bert_kernels_host.py proves the premises on the CPU.  Buffers start as NaN or as the poison
pattern of ops.poison, compared as integers, so that an element a kernel skipped or wrote where it should not shows."""
import pytest
import torch

import bert_kernels_util as B
import decode_gemm_util as U
from decode_gemm_util import int_a, int_bias, int_bits, int_product, int_w, rnd

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
_ID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_seen = {}                       # observed maxima of the fp64 comparisons, printed per test (recorded in the docstrings)


def _note(key, err):
    _seen[key] = max(_seen.get(key, 0.0), float(err))
    print(f"[{key}] max error so far {_seen[key]:.3e}")


@pytest.fixture(scope="module")
def ops():
    from mgea import ops as o
    return o


def _canary(ops, n, dtype=torch.float32):
    """n elements whose bits are ops.POISON_BITS (16-bit types: its upper half, a NaN in bf16 and fp16 alike)"""
    if dtype == torch.float32:
        return ops.poison(n, dtype, device="cuda")
    return torch.full((int(n),), ops.POISON_BITS >> 16, dtype=torch.int16, device="cuda").view(dtype)


def _is_poison(ops, t):
    return bool((int_bits(t.cpu()) == (ops.POISON_BITS if t.element_size() == 4 else ops.POISON_BITS >> 16)).all())


# ---- bert_embed_ln_kernel / bert_embed_ln_bf16_kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [0, 1], ids=["padded", "packed"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ID.get)
def test_bert_embed_against_fp64(ops, dtype, packed):
    """fp64 LayerNorm of word[id] + pos[t], eps 1e-12, at every D that changes the lane geometry (idle lanes at 128, a straggler float4
    at 1028, the largest D of each kernel) and row counts that are no multiple of the bf16 kernel's 4 rows per block; one word row
    carries a DC offset of +50 against a spread of 1.  f32: atol 2e-5; bf16: bf16_bound.
    Observed on MI355X: f32 1.3e-5, bf16 2.7e-6 beyond one rounding"""
    eps = 1e-12
    for D in B.EMBED_D[dtype]:
        for bs, (Bn, S) in enumerate(B.EMBED_BS if not packed else [(0, 0)]):
            ids, pos_ids, t = B.embed_ids(Bn, S, packed, seed=bs)
            word, pos, ln_w, ln_b = B.embed_tables(D, max(64, int(t.max()) + 1), seed=D)
            want = B.embed_ref(ids, t, word, pos, ln_w, ln_b, eps)
            out, flag = ops.bert_embed(ids.cuda(), word.cuda(), pos.cuda(), ln_w.cuda(), ln_b.cuda(), eps, dtype,
                                       pos_ids=None if pos_ids is None else pos_ids.cuda())
            got = out.double().cpu()
            assert flag == 0, "every id is valid: the flag word must stay 0"
            bound = torch.full_like(want, 2e-5) if dtype == torch.float32 else B.bf16_bound(want)
            err = (got - want).abs()
            _note(f"bert_embed {_ID[dtype]}", (err - (bound - 2e-5)).max() if dtype == torch.bfloat16 else err.max())
            bad = ~(err <= bound)
            assert not bad.any(), (f"D={D} B={Bn} S={S} packed={packed}: {int(bad.sum())} elements off, worst {float(err.max()):.3e} "
                                   f"(row {int(bad.nonzero()[0][0])}, id {int(ids.reshape(-1)[int(bad.nonzero()[0][0])])})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ID.get)
def test_bert_embed_clamps_and_reports_ids_outside_the_vocabulary(ops, dtype):
    """ids -1 and vocab are clamped to rows 0 / vocab - 1 and the flag word becomes 1; without a flag word the same rows come out"""
    D, eps = 128, 1e-12
    ids, _, t = B.embed_ids(3, 7, 0)
    ids[0, 2], ids[1, 0], ids[2, 6] = -1, B.VOCAB, B.VOCAB + 1000
    word, pos, ln_w, ln_b = (x.cuda() for x in B.embed_tables(D, 64, seed=5))
    clamped = ids.clamp(0, B.VOCAB - 1)
    want, flag0 = ops.bert_embed(clamped.cuda(), word, pos, ln_w, ln_b, eps, dtype)
    got, flag = ops.bert_embed(ids.cuda(), word, pos, ln_w, ln_b, eps, dtype)
    silent, none = ops.bert_embed(ids.cuda(), word, pos, ln_w, ln_b, eps, dtype, want_flag=False)
    assert flag0 == 0 and flag == 1 and none is None
    assert torch.equal(int_bits(got), int_bits(want)) and torch.equal(int_bits(silent), int_bits(want))
    ref = B.embed_ref(ids, t, *(x.cpu() for x in (word, pos, ln_w, ln_b)), eps)       # rows 0 / vocab - 1 for the three bad ids
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= (torch.full_like(ref, 2e-5) if dtype == torch.float32 else B.bf16_bound(ref))).all())


@pytest.mark.parametrize("dtype,D", [(torch.float32, 4100), (torch.bfloat16, 2052), (torch.float32, 10), (torch.bfloat16, 10)],
                         ids=lambda x: _ID.get(x, str(x)))
def test_bert_embed_refuses_rows_it_cannot_hold(ops, dtype, D):
    ids, _, _ = B.embed_ids(3, 7, 0)
    word, pos, ln_w, ln_b = (x.cuda() for x in B.embed_tables(D, 8, seed=1))
    out = _canary(ops, 21 * D, dtype)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.bert_embed(ids.cuda(), word, pos, ln_w, ln_b, 1e-12, dtype, out=out)
    torch.cuda.synchronize()
    assert _is_poison(ops, out), "a refused call wrote to its output"


# ---- gather_rows_kernel / gather_cls_bf16_kernel / gather_cls_ln_bf16_kernel ------------------------------------------------------
@pytest.mark.parametrize("packed", [0, 1], ids=["padded", "packed"])
@pytest.mark.parametrize("D", [128, 768])
def test_gather_cls_picks_the_first_row_of_every_sequence(ops, D, packed):
    """Rows that are not a [CLS] row are NaN: a wrong row index shows as NaN.  f32 and plain bf16: the selected rows bit for bit.
    LN form: fp64 ((h - mean) rstd) g + b at 2^-22 (|(h - mean) rstd g| + |b|): three fp32 roundings (subtract, two products, the last
    fused with the add) of 2^-24 each, plus slack.  Observed on MI355X: 0.50 of the bound"""
    Bn, S = 5, 7
    h, rowstat, g, be, cu, first = B.gather_inputs(Bn, S, D, packed, seed=D)
    cud = None if cu is None else cu.cuda()
    got = ops.gather_cls(h.cuda(), Bn, S, cu=cud).cpu()
    assert torch.equal(got, h[first]), "f32 gather"
    h16 = h.bfloat16()
    got = ops.gather_cls(h16.cuda(), Bn, S, cu=cud).cpu()
    assert torch.equal(got, h16[first].float()), "bf16 gather"
    got = ops.gather_cls(h16.cuda(), Bn, S, cu=cud, rowstat=rowstat.cuda(), ln_g=g.cuda(), ln_b=be.cuda()).double().cpu()
    core = (h16[first].double() - rowstat[first, 0:1].double()) * rowstat[first, 1:2].double() * g.double()
    want = core + be.double()
    bound = 2.0 ** -22 * (core.abs() + be.double().abs())
    err = (got - want).abs()
    _note("gather_cls LN / bound", (err / bound).max())
    assert bool((err <= bound).all()), f"LN gather: worst {float((err / bound).max()):.2f} of the bound"


# ---- layernorm_bf16_kernel<2> / <4> ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", B.LN16_C)
def test_layernorm_bf16_every_instantiation_against_fp64(ops, C):
    """<2> with the clamped chunk index (C < 512: 8, 128), with idle lanes in the second chunk (520, 768), full (1024); <4> (1032:
    one chunk past <2>; 2048: the largest C), M that is no multiple of the 4 rows per wave or 16 per block, out of place and in place.
    Reference: fp64 on the same bf16 input, bf16_bound.  Observed on MI355X: 1.1e-8 beyond one bf16 rounding"""
    from mgea import _lib
    w, b = (1 + 0.1 * rnd(C, seed=2)).cuda(), (0.1 * rnd(C, seed=3)).cuda()
    for M in B.LN16_M:
        x = (rnd(M, C, seed=M + C, scale=2.0) + 0.3).bfloat16()
        want = B.ln64(x, w.cpu(), b.cpu(), 1e-5)
        xd = x.cuda()
        got = ops.layernorm_bf16(xd, w, b, 1e-5)
        assert torch.equal(int_bits(xd.cpu()), int_bits(x)), "out of place: the input changed"
        inplace = xd.clone()
        _lib.check(_lib.load().mgea_op_layernorm_bf16(_lib.ptr(inplace), _lib.ptr(w), _lib.ptr(b), _lib.ptr(inplace), M, C, 1e-5,
                                                      _lib.stream_ptr()))
        assert torch.equal(int_bits(inplace.cpu()), int_bits(got.cpu())), f"M={M}: in place differs from out of place"
        err, bound = (got.double().cpu() - want).abs(), B.bf16_bound(want)
        _note("layernorm_bf16", (err - (bound - 2e-5)).max())
        bad = ~(err <= bound)
        assert not bad.any(), f"M={M} C={C}: {int(bad.sum())} elements off, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("C", [2056, 12])
def test_layernorm_bf16_refuses_rows_it_cannot_hold(ops, C):
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.layernorm_bf16(torch.zeros(4, C).bfloat16().cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda(), 1e-5)


# ---- bias_act_kernel<NONE / GELU / RELU> --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ldo", B.BIAS_ACT_SHAPES)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_GELU], ids=["none", "relu", "gelu"])
def test_slab_bias_act(ops, act, S, M, N, ldo):
    """Integer slabs (x 1/4 for GELU: arguments within +-12): none / relu equal the integer answer, GELU is held to fp64 erf-GELU at
    2e-5 (the bound of test_skinny_gemm_ln_gelu and test_gelu_poly).  N % 4 in {0, 1, 2}, ldo % 4 != 0 (scalar stores), ldo > N, a
    second grid column (N > 1024).  Columns N .. ldo - 1 and the canary behind the buffer stay as they were.
    Observed on MI355X (GELU): 3.5e-7"""
    scale = 0.25 if act == ACT_GELU else 1.0
    ldp = (N + 3) // 4 * 4 + 4
    P, bias = B.int_slabs(S, M, ldp, N), int_bias(N)
    exact = B.slab_sum(P, N, bias).double() * scale
    for with_bias in ([True, False] if (S, M) == (3, 5) else [True]):
        want = exact if with_bias else B.slab_sum(P, N).double() * scale
        if act == ACT_RELU:
            want = want.clamp(min=0)
        if act == ACT_GELU:
            assert float(want.abs().max()) <= 12
            want = B.gelu64(want)
        buf = _canary(ops, M * ldo + 64)
        out = buf[:M * ldo].view(M, ldo)[:, :N]
        ops.slab_bias_act((P * scale).cuda(), (bias * scale).cuda() if with_bias else None, out, act)
        got = buf.cpu()
        assert _is_poison(ops, got[M * ldo:]) and (ldo == N or _is_poison(ops, got[:M * ldo].view(M, ldo)[:, N:])), "wrote outside [M, N]"
        res = got[:M * ldo].view(M, ldo)[:, :N].double()
        if act == ACT_GELU:
            err = float((res - want).abs().max())
            _note("slab_bias_act gelu", err)
            assert err <= 2e-5, f"GELU off fp64 by {err:.3e}"
        else:
            assert torch.equal(res, want), f"{int((res != want).sum())} elements differ from the exact answer"


# ---- bias_res_ln_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", B.RES_LN_C)
@pytest.mark.parametrize("M", B.RES_LN_M)
@pytest.mark.parametrize("S", B.RES_LN_S)
def test_slab_bias_res_ln(ops, S, M, C):
    """pre-LN without LayerNorm: x = the integer sum exactly; pre-LN with it: x exact and xn = fp64 LayerNorm of that x at 2e-5 (the
    bound of test_layernorm); post-LN: x = that LayerNorm.  Observed on MI355X: 5.2e-7"""
    P, bias, x0 = B.int_slabs(S, M, C + 8, C), int_bias(C), B.int_x(M, C)
    ln_w, ln_b = 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2)
    total = B.slab_sum(P, C, bias) + x0.long()
    want_ln = B.ln64(total, ln_w, ln_b, 1e-5)
    Pd, bd = P.cuda(), bias.cuda()
    x, xn = ops.slab_bias_res_ln(Pd, bd, x0.cuda().clone())
    assert xn is None and torch.equal(x.cpu().long(), total) and torch.equal(x.cpu(), total.float())
    x, xn = ops.slab_bias_res_ln(Pd, None, x0.cuda().clone())
    assert torch.equal(x.cpu().double(), (B.slab_sum(P, C) + x0.long()).double()), "NULL bias"
    x, xn = ops.slab_bias_res_ln(Pd, bd, x0.cuda().clone(), ln_w.cuda(), ln_b.cuda(), 1e-5)
    assert torch.equal(x.cpu(), total.float()), "pre-LN: x must hold the exact sum"
    err = float((xn.double().cpu() - want_ln).abs().max())
    x, none = ops.slab_bias_res_ln(Pd, bd, x0.cuda().clone(), ln_w.cuda(), ln_b.cuda(), 1e-5, post_ln=True)
    err = max(err, float((x.double().cpu() - want_ln).abs().max()))
    _note("slab_bias_res_ln", err)
    assert none is None and err <= 2e-5, f"LayerNorm off fp64 by {err:.3e}"


def test_slab_bias_res_ln_refusals(ops):
    for C, kw, msg in [(128, dict(post_ln=True), "LayerNorm weights"), (4100, {}, "bad C")]:
        x = _canary(ops, 2 * C).view(2, C)
        with pytest.raises(RuntimeError, match=msg):
            ops.slab_bias_res_ln(B.int_slabs(1, 2, C).cuda(), int_bias(C).cuda(), x, **kw)
        torch.cuda.synchronize()
        assert _is_poison(ops, x)


# ---- logits_argmax_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", B.LOGITS_V)
@pytest.mark.parametrize("M", B.LOGITS_M)
@pytest.mark.parametrize("S", B.LOGITS_S)
def test_slab_logits_argmax(ops, S, M, V):
    """The logits are the exact integer sums; the argmax is the FIRST index of the row maximum: rows whose maximum is duplicated in
    columns that different waves scan, at the last column, and the natural rows (small integers: many ties).  Each output alone
    (the other pointer NULL) equals what the full call gives; an all -inf row gives index 0."""
    for shift in (0, 1):
        P, bias, L, first = B.argmax_slabs(S, M, V, shift)
        Pd, bd = P.cuda(), bias.cuda()
        new = lambda: (_canary(ops, M * V + 16), torch.full((M + 4,), -7, dtype=torch.int32, device="cuda"))
        lg, am = new()
        ops.slab_logits_argmax(Pd, bd, V, logits=lg, argmax=am)
        assert torch.equal(lg[:M * V].view(M, V).cpu().double(), L.double()) and _is_poison(ops, lg[M * V:]), "logits"
        assert am.cpu().tolist() == first + [-7] * 4, f"argmax {am.cpu().tolist()} expected {first}"
        lg2, am2 = new()
        ops.slab_logits_argmax(Pd, bd, V, argmax=am2)
        assert torch.equal(am2, am), "argmax with logits = NULL"
        ops.slab_logits_argmax(Pd, bd, V, logits=lg2)
        assert torch.equal(int_bits(lg2), int_bits(lg)), "logits with argmax = NULL"
    lg, am = new()
    ops.slab_logits_argmax(Pd, torch.full((V,), float("-inf")).cuda(), V, logits=lg, argmax=am)
    assert am.cpu().tolist() == [0] * M + [-7] * 4 and bool((lg[:M * V] == float("-inf")).all())


# ---- qkv_scatter_kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=_ID.get)
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("lens", [(3, 1), None], ids=["ragged", "full"])
@pytest.mark.parametrize("max_pages", [3, 2])
def test_slab_qkv_scatter(ops, max_pages, lens, dh, pdtype):
    """ctx_len [62, 130], T = 3: row 0 crosses a page boundary (62, 63 | 64), row 1 writes into logical page 2 -- cached with a table of
    3 pages, past the table and NOT cached with one of 2.  The page image starts as poison and must equal, bit for bit, the image
    ops.kv_pages_write builds on the host; qkv_out rows past lens are zero rows.  Both forms: slab sum + bias + qkv_out, and scatter
    only from the finished buffer."""
    H, Bn, T = 2, 2, 3
    P, bias, ctx_len, want = B.scatter_case(dh, lens, max_pages)
    n_pages = B.n_pages_for(Bn, max_pages)
    table = U.permuted_table(Bn, max_pages, n_pages)
    full = B.slab_sum(P, 3 * H * dh, bias).float()           # every row, also those past lens: the finished buffer of the second form
    expect = U.expected_image(ops, full, H, dh, table, ctx_len, lens, T, n_pages, 0, 1, pdtype)
    assert not _is_poison(ops, expect) and bool((int_bits(expect) == int_bits(ops.poison(1, pdtype))).any())
    args = (H, dh)
    tail = (torch.from_numpy(table).cuda(), torch.tensor(ctx_len).cuda(), None if lens is None else torch.tensor(lens).cuda(), T)
    pages = _canary(ops, expect.numel(), pdtype)
    out = ops.slab_qkv_scatter(P.cuda(), bias.cuda(), *args, pages, *tail)
    assert torch.equal(out.cpu().double(), want.double()), "qkv_out"
    assert torch.equal(int_bits(pages.cpu()), int_bits(expect)), "page image (slab form)"
    pages = _canary(ops, expect.numel(), pdtype)
    fin = torch.cat([full, torch.full((Bn * T, 8), float("nan"))], 1)[None].contiguous()
    assert ops.slab_qkv_scatter(fin.cuda(), None, *args, pages, *tail, want_qkv=False) is None
    assert torch.equal(int_bits(pages.cpu()), int_bits(expect)), "page image (scatter only)"


# ---- gemm_f32_nt_kernel: every split of K, and the direct epilogue ------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", B.GEMM_EXACT)
def test_gemm_f32_exact_at_every_split(ops, M, N, K):
    """integer operands: every split of K must give the int64 product bit for bit (test_gemm_f32 holds random operands to 2e-5)"""
    a, w, b = int_a(M, K), int_w(N, K), int_bias(N)
    want = int_product(a, w, b).double()
    ad, wd, bd = a.float().cuda(), w.float().cuda(), b.float().cuda()
    for split in sorted({min(s, K // 32) for s in B.GEMM_SPLITS}):
        got = ops.gemm(ad, wd, bd, split_k=split).cpu().double()
        assert torch.equal(got, want), f"split_k={split}: {int((got != want).sum())} of {M * N} elements differ"


@pytest.mark.parametrize("M,N,K", B.DIRECT_SHAPES)
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_GELU], ids=["none", "relu", "gelu"])
def test_gemm_f32_direct_epilogue(ops, act, M, N, K):
    """A is a column slice (lda = K + 32) and the output a column slice of a canary-filled matrix (ldo = N + 64, offset 32), as the
    last layer's K | V GEMM writes it; 1, 9 and 16 tiles (the last takes the XCD remap), N no multiple of the tile.  none / relu equal
    the int64 answer; every act is bitwise equal to the two-kernel form (same MFMA order, same gelu_erf); the canaries stay."""
    a, w, b = int_a(M, K), int_w(N, K), int_bias(N)
    abig = torch.full((M, K + 32), float("nan"))
    abig[:, 16:16 + K] = a.float()
    abig, wd, bd = abig.cuda(), w.float().cuda(), b.float().cuda()
    av = abig[:, 16:16 + K]
    big = _canary(ops, M * (N + 64) + 64)
    ops.gemm_direct(av, wd, bd, big[:M * (N + 64)].view(M, N + 64)[:, 32:32 + N], act)
    got = big.cpu()
    view = got[:M * (N + 64)].view(M, N + 64)
    assert _is_poison(ops, view[:, :32]) and _is_poison(ops, view[:, 32 + N:]) and _is_poison(ops, got[M * (N + 64):]), "canary columns"
    res = view[:, 32:32 + N]
    raw = ops.gemm(av, wd, None, split_k=1)
    two = torch.empty(M, N, device="cuda")
    ops.slab_bias_act(raw.view(1, M, N), bd, two, act)
    assert torch.equal(int_bits(res.contiguous()), int_bits(two.cpu())), "differs from GEMM + slab epilogue"
    if act != ACT_GELU:
        want = int_product(a, w, b).double()
        assert torch.equal(res.double(), want.clamp(min=0) if act == ACT_RELU else want)


def test_gemm_f32_direct_refusals(ops):
    z = lambda *s: torch.zeros(*s).cuda()
    for M, N, bias in [(64, 128, True), (65, 130, True), (65, 128, False)]:
        out = _canary(ops, M * N).view(M, N)
        with pytest.raises(RuntimeError, match="bad shape"):
            ops.gemm_direct(z(M, 32), z(N, 32), z(N) if bias else None, out)
        torch.cuda.synchronize()
        assert _is_poison(ops, out)


# ---- lora_merge_kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dim,in_dim,r", B.LORA_SHAPES)
def test_lora_merge(ops, out_dim, in_dim, r):
    """fp64 W + s B A at 2^-22 (|W| + s sum |B||A|): four roundings of 2^-24 of the sum of magnitudes (the kernel makes r + 2, each of a
    partial result that is far below that sum), and exact with integer W, A, B.  Observed on MI355X: 0.67 of the bound"""
    s = 2.0
    w, a, b = rnd(out_dim, in_dim, seed=1), rnd(r, in_dim, seed=2), rnd(out_dim, r, seed=3)
    got = ops.lora_merge(w.cuda(), a.cuda(), b.cuda(), s).double().cpu()
    want = w.double() + s * (b.double() @ a.double())
    bound = 2.0 ** -22 * (w.double().abs() + s * (b.double().abs() @ a.double().abs()))
    err = (got - want).abs()
    _note("lora_merge / bound", (err / bound).max())
    assert bool((err <= bound).all()), f"worst {float((err / bound).max()):.2f} of the bound"
    wi, ai, bi = B.int_x(out_dim, in_dim), int_a(r, in_dim).float(), int_w(out_dim, r).float()
    got = ops.lora_merge(wi.cuda(), ai.cuda(), bi.cuda(), s).cpu().double()
    assert torch.equal(got, wi.double() + s * (bi.double() @ ai.double()))
