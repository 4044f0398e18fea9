"""The fp16 instantiations behind the decoder's fp16 mode, one kernel at a time (mgea_op_* entry points with f16 operands).  The engine
tests hold them end to end at 4e-3 / 8e-3 on the logits, which a token in the wrong page slot or one lost key does not reach.  Here:
the KV page image is compared BITWISE with a host-built one (both are copies), the GEMM epilogues against fp64 on the same fp16
inputs at the bf16 bound / 8, the small kernels bitwise or at 1e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 0x5A5A            # every byte of a page pool before a kernel writes into it
CANARY = 4096            # elements in front of and behind the pool


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _i16(t):
    return t.view(torch.int16)


# ---- fp16 KV page image --------------------------------------------------------------------------------------------------------
class Pool:
    """n_pages fp16 pages on the device between two canary regions, every byte a sentinel; `want` is the host image the kernel's
    writes are expected to produce."""

    def __init__(self, n_pages, H, dh):
        from mgea import ops
        self.elems = ops.kv_page_elems(n_pages, H, dh)
        self.buf = torch.full((CANARY + self.elems + CANARY,), SENT, dtype=torch.int16, device="cuda").view(torch.float16)
        self.pages = self.buf[CANARY:CANARY + self.elems]
        self.want = torch.full((self.elems,), SENT, dtype=torch.int16).view(torch.float16)

    def check(self, what):
        buf = _i16(self.buf).cpu()
        assert bool((buf[:CANARY] == SENT).all()) and bool((buf[CANARY + self.elems:] == SENT).all()), f"{what}: wrote outside the pool"
        got, want = buf[CANARY:CANARY + self.elems], _i16(self.want)
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} of {self.elems} page elements differ from the host image, first at element "
                                  f"{int(bad[0])}: {int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x} (sentinel {SENT:#x})")


def _page_case(T, max_pages=None, seed=0):
    """B = 3, H = 2, dh = 64, prefix lengths [T, 1, 65]; a random permutation of a pool with more pages than the rows need"""
    B, H, dh = 3, 2, 64
    need = (T + 63) // 64
    max_pages = need if max_pages is None else max_pages
    n_pages = B * need + 5
    lens = torch.tensor([T, 1, min(65, T)])
    valid = torch.arange(T)[None, :] < lens[:, None]
    table = torch.from_numpy(np.random.RandomState(seed + T).permutation(n_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32))
    qkv = torch.randn(B, T, 3 * H * dh, generator=torch.Generator().manual_seed(seed + 1)).half()
    k, v = (qkv[..., i * H * dh:(i + 1) * H * dh].reshape(B, T, H, dh) for i in (1, 2))
    return B, H, dh, n_pages, lens, valid, table, qkv, k, v


@pytest.mark.parametrize("wide,pipe", [(0, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("T,max_pages", [(64, None), (129, None), (300, None), (300, 3)])
def test_f16_kv_page_image_is_bitwise_the_host_image(T, max_pages, wide, pipe, tune):
    """The in-kernel page write of the fp16 flash attention (a) and the scatter kernel with an empty cache (b) against the host-built
    image: every valid key's K | V bit for bit at its slot, every slot of an invalid key and every unused page still the sentinel,
    (a) == (b), and the attention output with pages bitwise the output without them.  max_pages = 3 at T = 300 (5 pages needed):
    tokens from 192 on are not cached and nothing outside the table's pages -- or the pool -- is touched."""
    from mgea import ops
    tune("attn16_wide", wide)
    tune("attn16_pipe", pipe)
    B, H, dh, n_pages, lens, valid, table, qkv, k, v = _page_case(T, max_pages)
    mask = valid.to(torch.int32).cuda()
    a, b = Pool(n_pages, H, dh), Pool(n_pages, H, dh)
    ops.kv_pages_write(a.want, k, v, table.numpy(), valid=valid.numpy())
    b.want = a.want
    assert int((_i16(a.want) != SENT).sum()) > 0
    out_pages = ops.attention16(qkv.cuda(), H, mask=mask, pages=a.pages, page_table=table.cuda())
    out_plain = ops.attention16(qkv.cuda(), H, mask=mask)
    a.check(f"attention16 with pages, T={T}")
    assert torch.equal(_i16(out_pages), _i16(out_plain)), "the attention output changes when the kernel also writes the pages"
    ops.kv_scatter_f16(qkv.cuda(), H, b.pages, table.cuda(), torch.zeros(B, dtype=torch.int32).cuda(), lens.cuda())
    b.check(f"kv_scatter_f16, T={T}")
    assert torch.equal(_i16(a.pages), _i16(b.pages))


def test_f16_kv_scatter_appends_across_a_page_boundary():
    """ctx_len = [0, 63, 64, 100] with 70 new tokens: the write of every row crosses a page, rows 1 and 3 start inside one."""
    from mgea import ops
    B, T, H, dh, max_pages = 4, 70, 2, 64, 3
    ctx = torch.tensor([0, 63, 64, 100])
    lens = torch.tensor([70, 70, 1, 37])
    valid = torch.arange(T)[None, :] < lens[:, None]
    n_pages = B * max_pages + 5
    table = torch.from_numpy(np.random.RandomState(5).permutation(n_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32))
    qkv = torch.randn(B, T, 3 * H * dh, generator=torch.Generator().manual_seed(2)).half()
    k, v = (qkv[..., i * H * dh:(i + 1) * H * dh].reshape(B, T, H, dh) for i in (1, 2))
    p = Pool(n_pages, H, dh)
    ops.kv_pages_write(p.want, k, v, table.numpy(), pos0=ctx.numpy(), valid=valid.numpy())
    ops.kv_scatter_f16(qkv.cuda(), H, p.pages, table.cuda(), ctx.cuda(), lens.cuda())
    p.check("kv_scatter_f16 with ctx_len")
    kk, vv = ops.kv_pages_read(p.pages.cpu(), table.numpy(), 3, 137, H, dh)            # and back through the reader
    assert torch.equal(_i16(kk[100:]), _i16(k[3, :37])) and torch.equal(_i16(vv[100:]), _i16(v[3, :37]))


@pytest.mark.parametrize("ragged", [False, True])
def test_f16_prefill_page_write_forms_are_bitwise_equal(ragged, tune):
    """Switch decoder_prefill16_pages: the fp16 prefill writes the KV pages from inside its attention kernel (1, default) or with the
    scatter kernel (0).  Both copy the same fp16 rows: bitwise-equal prefill logits and bitwise-equal logits of the first decode
    step, which reads those pages."""
    from mgea import synth
    from mgea.decoder import DecoderEngine
    sd, n_head = synth.decoder_state_dict(91, 300, 256, 256, 2), 4
    tune("decoder_prefill16", 2)
    B, T = 8, 256
    idx = torch.from_numpy(synth.integers(5, "p16", (B, T), 0, 300))
    lens = torch.tensor([T, 200, 256, 17, 129, 64, 255, 1]) if ragged else None
    outs = {}
    for form in (0, 1):
        tune("decoder_prefill16_pages", form)
        eng = DecoderEngine(sd, n_head=n_head, max_batch=B, max_ctx=T + 8, dtype="f16")
        lg = eng.reset_and_prefill(idx, lens).cpu()
        assert eng.stats()["prefill16_forwards"] == 1
        _, st = eng.step(None, eng.sampler(1.0, 1), want_logits=True)
        outs[form] = (lg, st.cpu())
        eng.close()
    real = torch.ones(B, T, dtype=torch.bool) if lens is None else torch.arange(T)[None, :] < lens[:, None]
    assert torch.equal(outs[0][0][real], outs[1][0][real]), "prefill logits differ between the two page-write forms"
    assert torch.equal(outs[0][1], outs[1][1]), "first decode step differs: the two forms left different KV pages"


# ---- fp16 GEMM epilogues -------------------------------------------------------------------------------------------------------
# One fp16 rounding is at most 2^-12 of the power of two below the value, up to 2^-11 = 4.9e-4 of the value itself: the bf16 bound of
# tests/test_gpu_bf16.py (BF16_REL = 4.3e-3, same arithmetic, 8 significand bits) divided by 8 for the three extra bits.
# Observed on MI355X over the first four shapes, the epilogues and phase schedules below: 3.2e-4 to 4.4e-4 (epilogues 3 / 4 / 5; the two
# shapes over 256 tiles pass the same bound, their maxima were not recorded); epilogue 6 (fp32
# output, bound 2e-5): 4.9e-7 and 7.3e-7; epilogue 5's statistics: tile sum 7.6e-6 (2e-3), tile M2 2.4e-7 relative (1e-4), merged mean
# 2.8e-8 (1e-5), rstd 8.2e-8 relative (1e-4).
F16_REL = 4.3e-3 / 8


def _ln_tables(M, seed):
    g = torch.Generator().manual_seed(seed)
    mean = (torch.rand(M, generator=g) * 2 - 1) * 0.3
    rstd = 0.5 + torch.rand(M, generator=g)
    return torch.stack([mean, rstd], 1).contiguous()


def _gemm_case16(M, N, K, epi, seed=21):
    """_gemm_case of tests/test_gpu_bf16.py on fp16 inputs, with the reference in fp64 (on the GPU: plain matmul)"""
    dev = "cuda"
    a = rnd(M, K, seed=seed).half().to(dev)
    w = rnd(N, K, seed=seed + 1, scale=K ** -0.5).half().to(dev)
    b = rnd(N, seed=seed + 2).to(dev)
    r = rnd(M, N, seed=seed + 3).half().to(dev)
    acc = a.double() @ w.double().t()
    kw, pre = {}, None
    if epi in (3, 4):
        st = _ln_tables(M, seed + 4).to(dev)
        c1 = w.float().sum(1)
        want = st[:, 1:2].double() * (acc - st[:, 0:1].double() * c1.double()) + b.double()
        if epi == 4:
            want = torch.nn.functional.gelu(want)
        kw.update(ln=dict(rowstat=st, c1=c1), gelu=epi == 4)
    else:
        st = _ln_tables(M, seed + 4).to(dev)
        g, be = (rnd(N, seed=seed + 5) * 0.2 + 1.0).to(dev), (rnd(N, seed=seed + 6) * 0.2).to(dev)
        pre = acc + b.double()
        want = pre + ((r.double() - st[:, 0:1].double()) * st[:, 1:2].double() * g.double() + be.double())
        kw.update(res=r, ln=dict(rowstat=st, g=g, b=be, stats=True))
    scale = want.abs() + 1.0 if pre is None else want.abs() + pre.abs() + 1.0
    return a, w, b, (want, scale), kw


# tiles of 256 x 256 -> what one XCD's run of them looks like on the 256 workgroups (32 per XCD) of an MI355X.  Up to 256 tiles every
# workgroup computes ONE whole tile whatever bf16_gemm_tail says (8, 18, 72 and 102 tiles: the issue's four shapes -- they cover the
# smallest accepted shape, ragged M, M % 256 == 128 and the epilogues' arithmetic, not the schedules).  306 tiles (XCD runs of 39 and
# 33 on 32 workgroups: 7 and 1 tiles left after the full round) and 297 tiles (38 / 31: 6 left, odd K-tile count 7) put a second
# whole tile on a workgroup -- the LDS-DMA stream continues over the tile boundary, the stage parity flips at odd K-tile counts --
# and end in half-tile units; at M = 8576 the last row tile's lower half starts AT row M and must not exist.
GEMM16_SHAPES = [(512, 1024, 64), (1300, 768, 192), (2048, 2304, 768), (8576, 768, 192), (8576, 2304, 768), (8448, 2304, 448)]
GEMM16_HALF_TILES = {(8576, 2304, 768), (8448, 2304, 448)}


@pytest.mark.parametrize("M,N,K", GEMM16_SHAPES)
@pytest.mark.parametrize("epi", [3, 4, 5])
@pytest.mark.parametrize("phases", [4, 2, 1])
def test_gemm_f16_folded_layernorm_epilogues(M, N, K, epi, phases, tune):
    """gemm_bf16_ph_kernel<EPI, _Float16, PH> on the shapes above, every phase schedule.  Every element against fp64 on the same fp16
    inputs; the launcher's report of half-tile units (info[1]) as expected per shape, so that the bitwise comparison of whole tiles /
    half tiles / staggered half tiles is known to compare different schedules where the shape has a tail; the row statistics of
    epilogue 5 against the statistics of the fp16 rows it wrote."""
    from mgea import ops
    tune("bf16_gemm_phases", phases)
    a, w, b, (want, scale), kw = _gemm_case16(M, N, K, epi)
    outs = {}
    for tail in (0, 1, 2):
        tune("bf16_gemm_tail", tail)
        info = []
        outs[tail] = ops.gemm_f16_ln(a, w, b, info=info, **kw)
        assert info == [2, int(tail != 0 and (M, N, K) in GEMM16_HALF_TILES)], info
    out, stats = outs[1] if epi == 5 else (outs[1], None)
    assert out.dtype == torch.float16
    err = float(((out.double() - want).abs() / scale).max())
    print(f"[gemm_f16_ln] M={M} N={N} K={K} epi={epi} phases={phases}: max err / scale = {err:.3e} (bound {F16_REL:.3e})")
    assert err < F16_REL
    for tail in (0, 2):
        o2, s2 = outs[tail] if epi == 5 else (outs[tail], None)
        assert torch.equal(o2, out), f"tail schedule {tail} differs bitwise"
        if epi == 5:
            assert torch.equal(s2, stats)
    if epi == 5:
        x = out.float().reshape(M, N // 256, 256)
        s1 = x.sum(-1)
        m2 = ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1)
        e_s1 = float((stats[..., 0] - s1).abs().max())
        e_m2 = float(((stats[..., 1] - m2).abs() / (m2 + 1.0)).max())
        rs = ops.ln_rowstat(stats, N, 1e-12)
        xd = out.double()
        e_mean = float((rs[:, 0].double() - xd.mean(1)).abs().max())
        e_rstd = float((rs[:, 1].double() * xd.var(1, unbiased=False).sqrt() - 1.0).abs().max())
        print(f"[gemm_f16_ln] rowstat: tile sum {e_s1:.2e} (2e-3), tile M2 rel {e_m2:.2e} (1e-4), mean {e_mean:.2e} (1e-5), rstd rel {e_rstd:.2e} (1e-4)")
        assert e_s1 < 2e-3 and e_m2 < 1e-4 and e_mean < 1e-5 and e_rstd < 1e-4


@pytest.mark.parametrize("M,N,K", [(512, 8324, 512), (1300, 1028, 256)])
def test_gemm_f16_fp32_output_head(M, N, K, tune):
    """Epilogue 6, the LM head of the fp16 prefill: fp32 [M, N] with N only a multiple of 4 (the last column tile is partial).
    fp16 products are exact in the fp32 accumulator: the project's fp32 GEMM bound, 2e-5.  A canary row behind the output stays.
    66 and 30 tiles: the last XCD's run is shorter than the others' and ends in half-tile units, so every phase schedule and every
    tail schedule runs, bitwise equal to the first."""
    from mgea import ops
    a = rnd(M, K, seed=41).half().cuda()
    w = rnd(N, K, seed=42, scale=K ** -0.5).half().cuda()
    b = rnd(N, seed=43).cuda()
    want = a.double() @ w.double().t() + b.double()
    first = None
    for phases in (2, 4, 1):
        tune("bf16_gemm_phases", phases)
        for tail in (2, 0, 1):
            tune("bf16_gemm_tail", tail)
            buf = torch.full((M + 1, N), -777.0, dtype=torch.float32, device="cuda")
            info = []
            out = ops.gemm_f16_ln(a, w, b, f32_out=True, info=info, out=buf[:M])
            assert info[0] == 2 and out.dtype == torch.float32
            assert bool((buf[M] == -777.0).all()), "the fp32 epilogue wrote past row M - 1"
            if first is None:
                first = out
                err = float((out.double() - want).abs().max())
                print(f"[gemm_f16_ln] epi 6 M={M} N={N} K={K}: max |out - fp64| = {err:.3e} (bound 2e-5)")
                assert err < 2e-5
            else:
                assert torch.equal(out, first), f"phases {phases} tail {tail} differs bitwise from the default schedule"


def test_gemm_f16_refuses_what_the_persistent_kernel_does_not_take():
    from mgea import ops
    K = 64
    for M, N, kw in [(256, 1024, {}), (512, 128, {}), (512, 1024, dict(no_c1=True))]:
        a, w, b = rnd(M, K, seed=1).half().cuda(), rnd(N, K, seed=2).half().cuda(), rnd(N, seed=3).cuda()
        st = _ln_tables(M, 4).cuda()
        c1 = None if kw.get("no_c1") else w.float().sum(1)
        out = torch.full((M, N), 7.0, dtype=torch.float16, device="cuda")
        with pytest.raises(RuntimeError) as ei:
            ops.gemm_f16_ln(a, w, b, ln=dict(rowstat=st, c1=c1), out=out)
        assert type(ei.value) is RuntimeError, f"MGEA_EINVAL expected, got {ei.value!r}"      # (MgeaError = a HIP / other failure)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call launched something"


# ---- the small kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [256, 768, 2048])
@pytest.mark.parametrize("absolute", [False, True])
def test_dec_embed_f16(C_, absolute):
    """x bitwise the fp16 RNE of the fp32 sum tok + pos; rowstat the (mean, rstd) of the ROUNDED row within 1e-5 of fp64; padded rows
    zero with (0, 1); the key mask; positions (absolute: + ctx_len) clamped at the last table row; ids clamped, flagged only when
    the token is real.  21 rows: not a multiple of the 4 rows per workgroup.  Observed on MI355X: mean 4.7e-9, rstd 1.3e-7."""
    from mgea import ops
    B, T, V, P, eps = 3, 7, 50, 5, 1e-5
    tok, pos = rnd(V, C_, seed=1), rnd(P, C_, seed=2)
    lens = torch.tensor([7, 3, 1])
    ctx = torch.tensor([0, 2, 1])
    ids = torch.from_numpy(np.random.RandomState(3).randint(0, V, size=(B, T)).astype(np.int32))
    ids[1, 5] = V + 9                                  # padding of row 1: clamped, NOT flagged
    ids[2, 3] = -4
    real = torch.arange(T)[None, :] < lens[:, None]
    for oov in (False, True):
        if oov:
            ids[0, 2], ids[1, 0] = V, -1               # real tokens: clamped to V - 1 / 0 and flagged
        x, rs, mk, flag = ops.dec_embed_f16(ids.cuda(), tok.cuda(), pos.cuda(), lens=lens.cuda(), ctx_len=ctx.cuda(), absolute_pos=absolute,
                                            eps=eps)
        assert flag == int(oov)
        p = torch.arange(T)[None, :] + (ctx[:, None] if absolute else 0)
        want = (tok[ids.long().clamp(0, V - 1)] + pos[p.clamp(max=P - 1)]).half()
        want[~real] = 0
        assert torch.equal(_i16(x.cpu()), _i16(want)), "x is not the fp16 rounding of the fp32 sum"
        assert torch.equal(mk.cpu(), real.to(torch.int32))
        xd = want.double()
        mean, rstd = xd.mean(-1), 1.0 / (xd.var(-1, unbiased=False) + eps).sqrt()
        rsc = rs.cpu().double()
        e_mean = float((rsc[..., 0] - mean)[real].abs().max())
        e_rstd = float((rsc[..., 1] - rstd)[real].abs().max())
        print(f"[dec_embed_f16] C={C_}: mean {e_mean:.2e}, rstd {e_rstd:.2e} (bound 1e-5)")
        assert e_mean < 1e-5 and e_rstd < 1e-5
        assert bool((rsc[..., 0][~real] == 0).all()) and bool((rsc[..., 1][~real] == 1).all())


@pytest.mark.parametrize("N,K", [(256, 768), (37, 200)])
def test_fold_ln_f16(N, K):
    from mgea import ops
    w, g, be, b = rnd(N, K, seed=1, scale=K ** -0.5), rnd(K, seed=2) * 0.3 + 1.0, rnd(K, seed=3) * 0.2, rnd(N, seed=4)
    wf, c1, c2 = ops.fold_ln_16(w.cuda(), g.cuda(), be.cuda(), b.cuda(), torch.float16)
    # ONE rounding of the exact product (48 significand bits: exact in fp64; numpy rounds fp64 -> fp16 directly): the kernel's
    # multiply-and-convert is a single v_fma_mixlo_f16.  Rounding the fp32 product again would differ on a few elements per thousand.
    exact = w.double().numpy() * g.double().numpy()[None, :]
    want = torch.from_numpy(exact.astype(np.float16))
    twice = (w * g[None, :]).half()
    print(f"[fold_ln f16] N={N} K={K}: {int((_i16(want) != _i16(twice)).sum())} of {N * K} elements tell one rounding from two")
    assert torch.equal(_i16(wf.cpu()), _i16(want))
    e1 = float((c1.cpu().double() - want.double().sum(1)).abs().max())
    e2 = float((c2.cpu().double() - (b.double() + w.double() @ be.double())).abs().max())
    print(f"[fold_ln f16] N={N} K={K}: c1 {e1:.2e}, c2 {e2:.2e} (bound 1e-5)")
    assert e1 < 1e-5 and e2 < 1e-5
    wb, c1b, c2b = ops.fold_ln_16(w.cuda(), g.cuda(), be.cuda(), b.cuda(), torch.bfloat16)      # the bf16 form IS fold_ln_bf16
    wb0, c1b0, c2b0 = ops.fold_ln_bf16(w.cuda(), g.cuda(), be.cuda(), b.cuda())
    assert torch.equal(_i16(wb), _i16(wb0)) and torch.equal(c1b, c1b0) and torch.equal(c2b, c2b0)


def test_f32_to_f16_is_round_to_nearest_even():
    from mgea import ops
    x = torch.cat([rnd(4100, seed=1, scale=3.0), rnd(1000, seed=2, scale=1e-6),          # normals, fp16 subnormals
                   torch.tensor([0.0, -0.0, 65504.0, 65519.9, 65520.0, -65520.0, 1e6, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24,
                                 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, float("inf")])])
    got = ops.f32_to_16(x.cuda(), torch.float16).cpu()
    assert torch.equal(_i16(got), _i16(x.half()))
    xb = x[torch.isfinite(x)]
    assert torch.equal(_i16(ops.f32_to_16(xb.cuda(), torch.bfloat16).cpu()), _i16(xb.bfloat16()))
