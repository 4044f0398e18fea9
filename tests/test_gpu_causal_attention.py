"""The two causal attention kernels alone, on inputs whose causal answer is known in closed form (tests/causal_util.py: latest, pointer,
prefix histogram; each held to fp64 causal softmax attention on the CPU).  A future key counted, the diagonal key lost, a key tile
skipped or a page too few moves an output by at least 1/8; the tolerance is the fp32 bound of the exact-answer tests, 2e-5.

dense  attn_dense_kernel<DH, CAUSAL> through mgea_op_attention_f32_causal: T around every 64-key tile boundary, several query blocks,
       no lens and ragged lens with 0 and 1, output into poison with a guard row, k-tiled output bitwise the row-major one, both
       grid walks (switch attn_causal_walk).
paged  attn_paged_kernel<dh + ATTN_PAGED_CAUSAL, ..> through mgea_op_attention_paged_causal: contexts 0 .. 200 ragged across the rows, T new tokens with
       ragged lens, fp32 and fp16 pages at every head_dim the launcher has, computed and table page ids, with and without the split
       scratch (T > 1 is never split and the causal form has no split kernel: info says 1, and the scratch's counters stay zero),
       k-tiled output, zero rows for padded queries.
causal=False calls of both ops are bitwise the calls they were."""
import numpy as np
import pytest
import torch

import causal_util as U

pytestmark = pytest.mark.gpu

MAX_PAGES = 8            # table width: > 4, so that a T = 1 launch with a scratch is split (the non-causal control)


def _guarded(n):
    """n floats of poison and a guard row of 256 behind them"""
    from mgea import ops
    buf = ops.poison(n + 256, device="cuda")
    return buf, buf[:n], buf[n:]


def _untouched(t):
    from mgea import ops
    return bool((t.view(torch.int32) == ops.POISON_BITS).all())


@pytest.mark.parametrize("kind", ["none", "ragged"])
@pytest.mark.parametrize("dh", U.DENSE_DH)
def test_dense_causal_sees_exactly_the_keys_up_to_the_query(dh, kind):
    from mgea import ops
    B, H, C = U.DENSE_B, U.DENSE_H, U.DENSE_H * dh
    for T in U.DENSE_T:
        lens = U.dense_lens(kind, T)
        l_dev = None if lens is None else torch.tensor(lens).cuda()
        for family in U.FAMILIES:
            case = U.dense_case(family, kind, T, dh)
            what = f"dense causal dh={dh} T={T} {kind} lens"
            _, out, guard = _guarded(B * T * C)
            ops.attention(case.qkv().cuda(), H, lens=l_dev, out=out, causal=True)
            assert _untouched(guard), f"{what} {family}: wrote behind the last row"
            out = out.view(B, T, C)
            case.check(out, what)
            if lens is not None:                       # the row of length 0: zero rows, the existing contract
                assert float(out[1].abs().max()) == 0.0, f"{what} {family}: the empty row is not zero"
            if B * T <= 512:                           # what a k-tiled buffer holds
                tiled = ops.attention(case.qkv().cuda(), H, lens=l_dev, tiled=True, causal=True)
                assert torch.equal(ops.untile_rows(tiled, B * T, C), out.view(B * T, C)), f"{what} {family}: tiled output differs"


@pytest.mark.parametrize("T", [65, 300, 1000])
def test_dense_causal_grid_walks_agree_bitwise(T, tune):
    """pairs-first (1, the default) and the non-causal kernel's block order (2) are the same workgroups in another order"""
    from mgea import ops, _lib
    assert _lib.tune_get("attn_causal_walk") == 1
    case = U.CausalCase("pointer", [T, 1, T - 1], [0, 0, 0], T, 2, 64)
    outs = []
    for walk in (1, 2):
        tune("attn_causal_walk", walk)
        outs.append(ops.attention(case.qkv().cuda(), 2, lens=torch.tensor([T, 1, T - 1]).cuda(), causal=True))
        case.check(outs[-1], f"walk {walk} T={T}")
    assert torch.equal(outs[0], outs[1])


def test_dense_causal_refuses_mask_and_packed_rows():
    """mask or cu with causal: the launcher's MGEA_EINVAL cannot be reached from outside the library -- mgea_op_attention_f32_causal is
    the _ex argument list WITHOUT mask and cu and passes NULL for both -- so what a caller can meet is the wrapper's RuntimeError (the
    exception MGEA_EINVAL maps to), raised before any library call so that a mask is never silently dropped.  The third assertion is
    another refusal of the same entry point, the library's own: a head_dim without a kernel."""
    from mgea import ops, _lib
    qkv = torch.zeros(2, 4, 3 * 64).cuda()
    with pytest.raises(RuntimeError, match="no mask"):
        ops.attention(qkv, 2, mask=torch.ones(2, 4, dtype=torch.int32).cuda(), causal=True)
    with pytest.raises(RuntimeError, match="no mask"):
        ops.attention(qkv.view(8, 192), 2, cu=torch.tensor([0, 4, 8]).cuda(), causal=True)
    # and the launcher itself, behind the wrapper: head_dim it has no kernel for is MGEA_EINVAL as in the non-causal form
    out = torch.zeros(2, 4, 64).cuda()
    rc = _lib.load().mgea_op_attention_f32_causal(_lib.ptr(qkv), None, _lib.ptr(out), 2, 4, 4, 16, 0, _lib.stream_ptr())
    assert rc == _lib.EINVAL


def test_non_causal_calls_are_the_calls_they_were():
    """causal=False goes to the entry points it always went to: bitwise the same outputs as the explicit non-causal ops"""
    from mgea import ops
    case = U.dense_case("latest", "ragged", 129, 64)
    lens = torch.tensor(U.dense_lens("ragged", 129)).cuda()
    a = ops.attention(case.qkv().cuda(), U.DENSE_H, lens=lens)
    b = ops.attention(case.qkv().cuda(), U.DENSE_H, lens=lens, causal=False)
    assert torch.equal(a, b)
    c = ops.attention(case.qkv().cuda(), U.DENSE_H, lens=lens, causal=True)
    assert not torch.equal(a[0], c[0])                # the mask does change the full row
    ctx = U.PAGED_CTX[1]
    pc = U.paged_case("pointer", ctx, 5, 64)
    outs = [_run_paged(pc, torch.float32, 0, True, ctx, 5, **kw)[0] for kw in (dict(), dict(causal=False))]
    assert torch.equal(outs[0], outs[1])


def _run_paged(case, pdtype, arith, split, ctx, T, causal=None, tiled=False):
    """-> (out [B, T, C], info, the scratch's counters): the keys ctx[b] + lens[b] of every row in pages, the rest of the image poison"""
    from mgea import ops
    B, H, dh = U.PAGED_B, case.H, case.dh
    lens = U.paged_lens(T)
    if arith:
        n_pages = MAX_PAGES * B
        table = np.arange(MAX_PAGES)[None, :] * B + np.arange(B)[:, None]
    else:
        n_pages = MAX_PAGES * B + 8
        table = np.random.RandomState(dh + T).permutation(n_pages)[:B * MAX_PAGES].reshape(B, MAX_PAGES)
    image = torch.empty(ops.kv_page_elems(n_pages, H, dh), dtype=pdtype)
    img = image.view(n_pages, 2, -1)
    img[:, 0] = 8.0
    img[:, 1] = 1024.0
    L = case.k.shape[1]
    valid = np.arange(L)[None, :] < case.n_keys[:, None]
    k, v = (torch.from_numpy(x).to(pdtype) for x in (case.k, case.v))
    ops.kv_pages_write(image, k, v, table, valid=valid)
    C = H * dh
    qkv = torch.zeros(B, T, 3 * C)
    qkv[..., :C] = torch.from_numpy(case.q.reshape(B, T, -1)).float()
    qkv[..., C:] = float("nan")                                     # the kernel reads K | V from the pages only
    scratch = ops.attn_split_scratch(dh) if split else None
    info = []
    kw = {} if causal is None else dict(causal=causal)
    out = ops.attention_paged(qkv.cuda(), H, image.cuda(), torch.from_numpy(table).cuda(), torch.tensor(list(ctx)).cuda(),
                              torch.tensor(lens).cuda(), arith_batch=B if arith else 0, split=split, info=info, scratch=scratch,
                              tiled=tiled, **kw)
    return out, info, None if scratch is None else scratch[1]


@pytest.mark.parametrize("ctx", U.PAGED_CTX, ids=lambda c: "ctx" + "_".join(map(str, c)))
@pytest.mark.parametrize("arith", [1, 0], ids=["arith", "table"])
@pytest.mark.parametrize("split", [0, 1], ids=["no_scratch", "scratch"])
@pytest.mark.parametrize("pdtype,dh", [(torch.float32, 32), (torch.float32, 64), (torch.float32, 96), (torch.float32, 128),
                                       (torch.float16, 32), (torch.float16, 64), (torch.float16, 128)],
                         ids=lambda x: {torch.float32: "f32", torch.float16: "f16"}.get(x, str(x)))
def test_paged_causal_sees_the_cache_and_the_new_tokens_up_to_the_query(pdtype, dh, split, arith, ctx):
    from mgea import ops
    for T in U.PAGED_T:
        lens = np.asarray(U.paged_lens(T))
        for family in U.FAMILIES:
            case = U.paged_case(family, ctx, T, dh)
            what = f"paged causal dh={dh} ctx={ctx} T={T} split={split} arith={arith}"
            out, info, count = _run_paged(case, pdtype, arith, bool(split), ctx, T, causal=True)
            assert info == [1], f"{what}: workgroups per query {info} (T > 1 is never split)"
            if count is not None:
                assert int(count.abs().max()) == 0, f"{what}: the split scratch's counters are not zero after the launch"
            case.check(out, f"{what} {family}")
            pad = torch.from_numpy(np.arange(T)[None, :] >= lens[:, None]).cuda()
            assert float(out[pad].abs().max()) == 0.0, f"{what} {family}: a padded query's row is not zero"
            if family == "pointer":
                tiled, _, _ = _run_paged(case, pdtype, arith, bool(split), ctx, T, causal=True, tiled=True)
                C = case.H * dh
                assert torch.equal(ops.untile_rows(tiled, U.PAGED_B * T, C), out.view(-1, C)), f"{what}: tiled output differs"


def test_paged_causal_single_token_is_the_decode_launch():
    """T == 1: t + 1 == n_new, the launcher takes the kernels a step always took -- split with a scratch, bitwise the non-causal call"""
    from mgea import ops
    ctx = (199, 64, 0, 63)
    B, H, dh = U.PAGED_B, U.PAGED_H, 64
    case = U.CausalCase("pointer", [c + 1 for c in ctx], list(ctx), 1, H, dh)
    image = torch.empty(ops.kv_page_elems(MAX_PAGES * B, H, dh))
    image.view(MAX_PAGES * B, 2, -1)[:, 0] = 8.0
    image.view(MAX_PAGES * B, 2, -1)[:, 1] = 1024.0
    table = np.arange(MAX_PAGES)[None, :] * B + np.arange(B)[:, None]
    L = case.k.shape[1]
    ops.kv_pages_write(image, torch.from_numpy(case.k).float(), torch.from_numpy(case.v).float(), table,
                       valid=np.arange(L)[None, :] < case.n_keys[:, None])
    qkv = torch.zeros(B, 1, 3 * H * dh)
    qkv[..., :H * dh] = torch.from_numpy(case.q.reshape(B, 1, -1)).float()
    outs = []
    for causal in (False, True):
        info, scratch = [], ops.attn_split_scratch(dh)
        outs.append(ops.attention_paged(qkv.cuda(), H, image.cuda(), torch.from_numpy(table).cuda(), torch.tensor(list(ctx)).cuda(),
                                        None, arith_batch=B, info=info, scratch=scratch, causal=causal))
        assert info == [ops.attn_split_count(B, H, 1, MAX_PAGES)] and info[0] > 1
        assert int(scratch[1].abs().max()) == 0
        case.check(outs[-1], f"T=1 causal={causal}")
    assert torch.equal(outs[0], outs[1])
