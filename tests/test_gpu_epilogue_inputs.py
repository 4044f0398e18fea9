"""The decode GEMMs' epilogue inputs -- bias, c1, the residual tile, the KV page id, the head's bias, the tail's row records: wherever
a kernel requests them (the tail loads the records with the row's state; QKV computes the page id where the pool carries the
allocation rule), each must still belong to its own element.  Everything goes through mgea_op_decode_gemm / mgea_op_step_tail
(test-only entries), one launch at a time.

RES cases are EXACT and every input names its element: A[m,k] = ((29 m + 13 k) mod 7) - 3, W[n,k] = w0[k] + d[n,k] with
w0[k] = ((71 k) mod 17) - 8 and d[n,k] = 1 where k mod 128 == (37 n) mod 128, bias[n] = n, residual[m,n] = m N + n.  All are
integers, every partial sum stays below 2^24 (|A W^T| <= 27 K <= 55 296, bias < 512, residual < 65 536), so the fp32 result is the
int64 one in any order.  A residual float4 taken from another row, column or pass moves the result by the distance of the two elements;
a bias from another column by the distance of the columns.
The tile statistics are exact too: inside a 16-column tile the result varies only by A[m] . (d[n] - d[n']) + 2 (n - n'), a few dozen
around the tile mean (a multiple of 1/16), so every squared distance is a multiple of 2^-8 and their sum M2 stays below 2^16
(exact_stats asserts it for every case): M2, every square and every partial sum of them have <= 24 significant bits, and (mean, M2)
in fp32 equals the fp64 value bit for bit in any order.  (The doubled launch moves further: its statistics are
held to the project's 1e-4 on powers-of-two-scaled operands elsewhere; here only its values are asserted.)

LayerNorm cases (ACT, QKV) use the operand distribution and the 2e-5 bound of tests/test_gpu_decode_gemm.py against fp64; c1 and c2
come from ops.fold_ln on random gamma / beta and are not constant.  No row has zero variance."""
import numpy as np
import pytest
import torch

import decode_gemm_util as U
import step_tail_util as S
from decode_gemm_util import DG_HEAD, DG_SKINNY, EPI_ACT, EPI_LOGITS, EPI_QKV, EPI_RES

pytestmark = pytest.mark.gpu

TOL = 2e-5   # tests/test_gpu_ops.py: fp32 GEMM / LayerNorm / GELU against fp64


@pytest.fixture(scope="module")
def ops():
    from mgea import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _ops


# ---- RES ---------------------------------------------------------------------------------------------------------------------------
def named_w(N, K):
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return ((71 * k) % 17 - 8) + (k % 128 == (37 * n) % 128).long()


def named_bias(N):
    return torch.arange(N)


def named_res(M, N):
    return torch.arange(M)[:, None] * N + torch.arange(N)[None, :]


def poisoned_tiled(ops, rows, N):
    """k-tiled buffer of whole 64-row groups: `rows` [M, N] on top, the poison bit pattern in the rows behind them"""
    M = rows.shape[0]
    R = (M + 63) // 64 * 64
    full = ops.poison(R * N).view(R, N).clone()
    full[:M] = rows
    return ops.tile_rows(full.cuda()), R


def exact_stats(v):
    """(mean, M2) of every 16-column tile in fp64 -> fp32 (exact by the module's premise) [M, N / 16, 2]"""
    t = v.double().reshape(v.shape[0], -1, 16)
    mean = t.mean(-1)
    m2 = ((t - mean[..., None]) ** 2).sum(-1)
    out = torch.stack([mean, m2], -1)
    # M2 < 2^16 is a sum of 16 non-negative multiples of 2^-8: it, every square and every partial sum of them have <= 24 bits
    assert bool((out.float().double() == out).all()) and float(m2.max()) < 2 ** 16, "the statistics are not exact in fp32: the premise of the test is broken"
    return out.float()


def first_diff(got, want):
    at = torch.nonzero(got != want)
    if at.numel() == 0:
        return "equal"
    m, n = (int(v) for v in at[0])
    return f"{at.shape[0]} elements differ, first at row {m} column {n}: got {float(got[m, n])} want {float(want[m, n])} (off by {float(got[m, n] - want[m, n])})"


RES_OPERANDS = {}


def res_operands(M, N, K):
    """computed once per shape and shared (the int64 product included); never modified"""
    if (M, N, K) not in RES_OPERANDS:
        a, w, b, r = U.int_a(M, K), named_w(N, K), named_bias(N), named_res(M, N)
        RES_OPERANDS[(M, N, K)] = (a, w, b, r, U.int_product(a, w, b))
    return RES_OPERANDS[(M, N, K)]


@pytest.mark.parametrize("N,K,nch", [(512, 512, 2), (512, 2048, 8)])
@pytest.mark.parametrize("M", [3, 16, 37, 64, 100])
def test_residual_bias_and_product_land_on_their_element(ops, M, N, K, nch):
    """out-projection and FC2 shapes: 16-row tiles, 8 waves, compile-time streams of 2 and 8 chunks; a partial row tile (3, 37, 100)
    and a second 64-row group (100).  Rows >= M of the residual and of the statistics stay as they were.  A second launch on the
    same buffer adds the product again: x + 2 (A W^T + b)."""
    a, w, b, r, prod = res_operands(M, N, K)
    at, _ = poisoned_tiled(ops, a.float(), K)           # rows >= M of A hold NaNs: their products are never stored
    wt, bd = ops.tile_weights(w.float().cuda()), b.float().cuda()
    x, R = poisoned_tiled(ops, r.float(), N)
    SR = max(64, M)
    stats = ops.poison(SR * (N // 16) * 2, device="cuda")
    _, ex, plan = ops.decode_gemm(EPI_RES, at, wt, bd, M, N, K, out=x, stats_out=stats)
    assert (plan["kind"], plan["mt"], plan["nt"], plan["nw"], plan["nch"]) == (DG_SKINNY, 1, 1, 8, nch), plan
    want = (prod + r).float()
    got = ops.untile_rows(x, R, N).cpu()
    assert torch.equal(got[:M], want), first_diff(got[:M], want)
    assert bool((U.int_bits(got[M:]) == ops.POISON_BITS).all()), "rows >= M of the residual were written"
    sgot = stats.cpu().view(SR, N // 16, 2)
    swant = exact_stats(want)
    assert torch.equal(U.int_bits(sgot[:M]), U.int_bits(swant)), first_diff(sgot[:M].reshape(M, -1), swant.reshape(M, -1))
    assert bool((U.int_bits(sgot[M:]) == ops.POISON_BITS).all()), "statistics of rows >= M were written"
    ops.decode_gemm(EPI_RES, at, wt, bd, M, N, K, out=x, stats_out=stats)
    want2 = (2 * prod + r).float()
    got = ops.untile_rows(x, R, N).cpu()
    assert torch.equal(got[:M], want2), "second launch on the same buffer: " + first_diff(got[:M], want2)
    assert bool((U.int_bits(got[M:]) == ops.POISON_BITS).all()), "rows >= M of the residual were written by the second launch"


# ---- ACT and QKV with the folded LayerNorm -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 37, 64])
def test_layernorm_act_takes_c1_and_c2_of_its_own_columns(ops, M):
    """FC1's shape (2048, 512), GELU: 32-row tiles, c1 [N] and c2 [N] (the bias slot) non-constant"""
    N, K = 2048, 512
    x, w, b, g, be = U.ln_operands(M, N, K, seed=900 + M)
    wd, c1, c2 = ops.fold_ln(w.cuda(), g.cuda(), be.cuda(), b.cuda())
    assert float(c1.std()) > 1e-3 and float(c2.std()) > 1e-3
    out, _, plan = ops.decode_gemm(EPI_ACT, ops.tile_rows(x.cuda()), wd, c2, M, N, K, act=1, ln_c1=c1, stats_in=U.tile_stats(x).cuda())
    assert (plan["kind"], plan["mt"], plan["nw"], plan["nch"]) == (DG_SKINNY, 1 if M <= 16 else 2, 8, 2), plan
    err = float((ops.untile_rows(out, M, N).cpu().double() - U.gelu64(U.ln_gemm64(x, w, b, g, be))).abs().max())
    print(f"LN-ACT M={M}: max |diff| {err:.3e}")
    assert err < TOL, err


def run_qkv(ops, M, C, dh, ctx, table, n_pages, arith_batch, seed, passed_table=None):
    """one T = 1 QKV launch: (qkv_out against fp64, the device image against the host image of the launch's own K | V at the pages
    `table` names); passed_table: what the kernel is given as its page table, if not `table`"""
    H, N, K = C // dh, 3 * C, C
    x, w, b, g, be = U.ln_operands(M, N, K, seed=seed)
    wd, c1, c2 = ops.fold_ln(w.cuda(), g.cuda(), be.cuda(), b.cuda())
    assert float(c1.std()) > 1e-3 and float(c2.std()) > 1e-3
    pages = ops.poison(2 * ops.kv_page_elems(n_pages, H, dh), device="cuda")
    kv = dict(pages=pages, n_pages=n_pages, n_head=H, head_dim=dh, layer=1, page_table=torch.from_numpy(table if passed_table is None else passed_table).cuda(),
              ctx_len=torch.tensor(ctx).cuda(), arith_batch=arith_batch)
    out, _, plan = ops.decode_gemm(EPI_QKV, ops.tile_rows(x.cuda()), wd, c2, M, N, K, ln_c1=c1, stats_in=U.tile_stats(x).cuda(), kv=kv)
    assert (plan["kind"], plan["mt"], plan["nw"], plan["nch"]) == (DG_SKINNY, 1 if M <= 16 else 2, 8, 2), plan
    err = float((out.cpu().double() - U.ln_gemm64(x, w, b, g, be)).abs().max())
    exp = U.expected_image(ops, out, H, dh, table, ctx, None, 1, n_pages, 1, 2, torch.float32)
    return err, torch.equal(U.int_bits(pages.cpu()), U.int_bits(exp))


@pytest.mark.parametrize("M", [3, 37, 64])
def test_layernorm_qkv_takes_c1_and_c2_of_its_own_columns(ops, M):
    """QKV's shape (1536, 512) on a permuted table"""
    ctx = [(7 * i) % 120 for i in range(M)]
    err, same = run_qkv(ops, M, 512, 64, ctx, U.permuted_table(M, 2, 2 * M + 1, mult=5 if (2 * M + 1) % 5 else 7), 2 * M + 1, 0, seed=950 + M)
    print(f"LN-QKV M={M}: max |diff| {err:.3e}")
    assert err < TOL, err
    assert same, "device page image differs from the host image"


@pytest.mark.parametrize("rule", [True, False], ids=["allocation_rule", "permuted_table"])
@pytest.mark.parametrize("M", [3, 64])
def test_qkv_page_scatter_by_rule_and_by_table(ops, M, rule):
    """Contexts 63, 64 and 65 (the new token is a page's last slot, the next page's first, its second).  (a) the pool carries the
    decoder's allocation rule, page j of row b = j * arith_batch + b: the kernel computes the id.  Run twice: with a table that
    repeats the rule, and with one whose every entry names the spare page -- a kernel that still looked the id up would put every
    row there (test-only: a real caller's table agrees with the rule);
    (b) no rule and a permuted table: the kernel looks it up.  Either way every K | V float4 lands in the page the table names and
    no other word of the poisoned two-layer image changes (one spare page no row owns included)."""
    ctx = [63 + i % 3 for i in range(M)]
    n_pages = 2 * M + 1
    if rule:
        table = (np.arange(2)[None, :] * M + np.arange(M)[:, None]).astype(np.int32)
    else:
        table = U.permuted_table(M, 2, n_pages, mult=5 if n_pages % 5 else 7, add=2)
    err, same = run_qkv(ops, M, 512, 64, ctx, table, n_pages, M if rule else 0, seed=970 + M)
    assert err < TOL, err
    assert same, "device page image differs from the host image"
    if rule:
        spare = np.full_like(table, n_pages - 1)
        err, same = run_qkv(ops, M, 512, 64, ctx, table, n_pages, M, seed=970 + M, passed_table=spare)
        assert err < TOL, err
        assert same, "with the allocation rule the page id must not come from the table"


# ---- head --------------------------------------------------------------------------------------------------------------------------
def head_partials(logits, G, base, n_extra):
    """head_balanced_kernel's per-workgroup (max, first index) partials [M, G] (csrc/head_gemm.hip): workgroup g owns the column tiles
    g * base .. of every row and, if g < n_extra, column tile G * base + g / 4 for the rows of row tile g % 4"""
    M, N = logits.shape
    val = torch.full((M, G), -float("inf"))
    idx = torch.full((M, G), 0x7FFFFFFF, dtype=torch.long)
    for g in range(G):
        spans = [(0, M, 16 * g * base, min(16 * (g + 1) * base, N))]
        if g < n_extra:
            j, r = G * base + g // 4, g % 4
            spans.append((16 * r, min(16 * r + 16, M), 16 * j, min(16 * j + 16, N)))
        for r0, r1, c0, c1 in spans:
            if r0 >= r1 or c0 >= c1:
                continue
            sub = logits[r0:r1, c0:c1]
            v = sub.max(1).values
            i = torch.where(sub == v[:, None], torch.arange(c0, c1)[None, :], torch.tensor(0x7FFFFFFF)).min(1).values
            better = v > val[r0:r1, g]          # the extra tile's columns lie above the own ones: a tie keeps the lower index
            val[r0:r1, g] = torch.where(better, v, val[r0:r1, g])
            idx[r0:r1, g] = torch.where(better, i, idx[r0:r1, g])
    return val, idx


@pytest.mark.parametrize("M", [3, 64])
def test_head_bias_lands_on_its_column(ops, M):
    """head_balanced_kernel<2, 2>: N = 8324, K = 512, bias a permutation of -4162 .. 4161 (every column its own value): logits
    and the per-workgroup (max, index) partials exact"""
    N, K = 8324, 512
    a, w = U.int_a(M, K), U.int_w(N, K)
    b = (7919 * torch.arange(N)) % N - N // 2
    assert len(set(b.tolist())) == N
    want = U.int_product(a, w, b).float()
    out, ex, plan = ops.decode_gemm(EPI_LOGITS, ops.tile_rows(a.float().cuda()), ops.tile_weights(w.float().cuda()), b.float().cuda(), M, N, K)
    assert (plan["kind"], plan["base"], plan["nch"]) == (DG_HEAD, 2, 2) and plan["n_partials"] == plan["grid_x"], plan
    assert torch.equal(out.cpu(), want), first_diff(out.cpu(), want)
    G, R = plan["grid_x"], ex["R"]
    n_extra = 4 * ((N + 15) // 16 - 2 * G)
    assert 0 < n_extra <= G
    val, idx = head_partials(want, G, 2, n_extra)
    p = ex["partials"].cpu()
    gval = p[: R * G].view(R, G)[:M]
    gidx = p[R * G: 2 * R * G].view(torch.int32).view(R, G)[:M].long()
    assert torch.equal(gval, val), first_diff(gval, val)
    assert torch.equal(gidx, idx), first_diff(gidx, idx)
    assert ops.merge_partials(ex["partials"], M, R, G).tolist() == U.first_argmax(want)


# ---- tail --------------------------------------------------------------------------------------------------------------------------
def test_tail_rows_stop_by_their_own_records(ops):
    """argmax_advance_embed_kernel, rows with records, one launch: row 0 stops on its EOS id (7, the by-value EOS 2 does not hold),
    row 1 on max_new, row 2 is parked at ctx_cap, row 3 runs on past another row's EOS id.  State by the written rule of
    tests/step_tail_util.py; the next embedding row at the position the rule leaves."""
    from mgea import _lib
    from mgea.decoder import RowSampling
    B, C, vocab, pos_rows, n_steps = 4, 128, 50, 64, S.N_STEPS
    sc = dict(tok=np.array([7, 11, 9, 7]), step=np.array([1, 2, 3, 1]), fed=np.array([40, 41, 42, 43]), len=np.array([10, 20, 30, 12]),
              done=np.zeros(4, np.int64), eos=np.array([7, -1, 9, 5]), max_new=np.array([0, 3, 0, 0]), cap=np.array([S.NONE, S.NONE, 31, S.NONE]))
    ex = S.expected_state(sc, True, n_steps=n_steps)
    assert ex["done"].tolist() == [1, 1, 2, 0] and ex["ctx_len"].tolist() == [11, 21, 30, 13] and ex["n_done"] == 3
    assert [sorted(t & {"eos", "budget", "park", "finish", "runs_on"}) for t in ex["tags"]] == \
        [["eos", "finish"], ["budget", "finish"], ["eos", "park"], ["runs_on"]]

    def dev(v):
        return torch.from_numpy(np.asarray(v, np.int64).astype(np.int32)).cuda()
    g = torch.Generator().manual_seed(77)
    tok_emb, pos_emb = torch.randn(vocab, C, generator=g), torch.randn(pos_rows, C, generator=g)
    n_tiles = 3
    pval = torch.tensor([[0.0, 5.0, 1.0]] * B)
    pidx = torch.stack([torch.tensor([int(t) + 1, int(t), int(t) + 2]) for t in sc["tok"]]).int()
    rows = [RowSampling(1.0, 1, None, None, int(sc["eos"][j]), int(sc["max_new"][j]), 0) for j in range(B)]
    st = dict(cur_ids=dev(sc["fed"]), ctx_len=dev(sc["len"]), done=dev(sc["done"]), row_step=dev(sc["step"]),
              n_done=torch.tensor([5], dtype=torch.int32).cuda(), ids_out=torch.full((B * n_steps,), S.POISON, dtype=torch.int32).cuda(), n_steps=n_steps)
    sampled = torch.full((B,), S.POISON, dtype=torch.int32).cuda()
    x, stats = ops.poison(ops.tiled_floats(B, C), device="cuda"), ops.poison(4 * B, device="cuda")
    embed = dict(tok_emb=tok_emb.cuda(), pos_emb=pos_emb.cuda(), x=x, stats=stats, C=C, vocab=vocab, pos_rows=pos_rows, absolute_pos=1)
    ops.step_tail(_lib.TAIL_ARGMAX_EMBED, B, st, rows=rows, ctx_cap=[int(c) for c in sc["cap"]], eos_id=S.EOS,
                  partials=(pval.cuda(), pidx.cuda(), n_tiles), sampled=sampled, embed=embed)
    assert sampled.cpu().tolist() == sc["tok"].tolist()
    for k in ("cur_ids", "ctx_len", "done", "row_step"):
        assert st[k].cpu().tolist() == ex[k].tolist(), k
    assert int(st["n_done"].cpu()) == 5 + ex["n_done"]
    assert st["ids_out"].cpu().view(B, n_steps).tolist() == ex["ids_out"].tolist()
    want = tok_emb[[S.embed_id(int(f), vocab) for f in ex["fed"]]] + pos_emb[[S.embed_position(int(n), 1, pos_rows) for n in ex["next_len"]]]
    got = ops.untile_rows(x, 64, C).cpu()
    assert torch.equal(got[:B], want), first_diff(got[:B], want)
    assert bool((U.int_bits(got[B:]) == ops.POISON_BITS).all()), "rows >= B of x were written"
