"""Paged attention: every element of q reaches the multiply-add of ITS dimension.

The pointer family of tests/test_gpu_attention_exact.py repeats each index bit over dh // 10 dimensions: a q element delivered to
the wrong dimension (or taken from the wrong lane) inside such a group changes no score.  Here every dimension stands alone:

  one-hot dimension   K[t] = e_(t mod dh) and q = beta * e_d: key t scores beta / sqrt(dh) >= 20 when t mod dh == d and 0
                      otherwise, so the softmax is uniform over the keys with t mod dh == d (over all keys when the row has
                      none) and out = the mean of their V rows -- multiples of 1/8, as in that file: exact in fp32 up to one
                      rounding.  q[d] multiplied with any other dimension of K picks another key set and moves the output by O(1).

Every d in turn, every head dimension the kernel is built for, contexts around the 64-token page, B = 2 and H = 2 (the row stride
3 C and the head offset of the q address), T = 1 and a ragged T = 3 (one row shorter than T: its padded query rows are zero), fp32
and fp16 pages, computed and table page ids, the plain and the split grid.  The inputs are held to fp64 softmax attention on the CPU
(1e-6) first -- that assertion is the condition on the inputs; the kernel then has 2e-5, that file's fp32 ulp.  On fp32 pages at
T = 1 the split grid must also equal the plain grid bit for bit on every row whose pages all belong to the first split."""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_attention_exact import MAX_PAGES, ULP, _page_setup, _ref64, _v_rows

pytestmark = pytest.mark.gpu

B, H = 2, 2
TOL = ULP[torch.float32]                                   # 2e-5
_ID = {torch.float16: "f16pages", torch.float32: "f32pages"}


def _beta(dh):
    """smallest power of two with a scaled score gap beta / sqrt(dh) >= 20"""
    return 2.0 ** math.ceil(math.log2(20.0 * math.sqrt(dh)))


def _contexts(dh):
    return [1, 63, 64, 65, 2 * dh + 1]


@functools.lru_cache(maxsize=None)
def _keys(totals, dh):
    """k, v [B, L, H, dh] (fp64) and valid [B, L] for rows that see totals[b] tokens"""
    L = max(totals)
    valid = np.arange(L)[None, :] < np.asarray(totals)[:, None]
    k = np.zeros((B, L, H, dh))
    k[:, np.arange(L), :, np.arange(L) % dh] = 1.0
    return k, _v_rows(B, L, H, dh), valid


def _queries(dims, dh):
    """dims [B, T, H] -> q [B, T, H, dh] = beta * e_dims"""
    q = np.zeros(dims.shape + (dh,))
    np.put_along_axis(q, dims[..., None], _beta(dh), axis=-1)
    return q


def _closed_form(dims, v, valid, dh):
    """mean V over the row's keys with t mod dh == d (all of its keys when there is none)"""
    out = np.empty(dims.shape + (dh,))
    t = np.arange(valid.shape[1])
    for b, i, h in np.ndindex(*dims.shape):
        hot = valid[b] & (t % dh == dims[b, i, h])
        out[b, i, h] = v[b, hot if hot.any() else valid[b], h].mean(0)
    return out


def _rounds(T, dh):
    """dims [B, T, H] per launch: every dimension in turn, twice -- the second time in another (row, head) slot"""
    per = B * T * H
    n = (dh + per - 1) // per
    base = np.arange(per).reshape(B, T, H)
    return [(base + per * r) % dh for r in range(n)] + [(base[::-1, :, ::-1] + per * r + 1) % dh for r in range(n)]


def _launch(q, image, table, ab, ctx_len, lens, split, T):
    from mgea import ops
    qkv = torch.zeros(B, T, 3 * H * q.shape[-1])
    qkv[..., :H * q.shape[-1]] = torch.from_numpy(q.reshape(B, T, -1)).float()
    qkv[..., H * q.shape[-1]:] = float("nan")                       # the kernel reads K | V from the pages only
    info = []
    out = ops.attention_paged(qkv.cuda(), H, image, table, ctx_len, lens, arith_batch=ab, split=split, info=info)
    assert info == [4 if split and T == 1 else 1], f"workgroups per query: {info}"
    return out.cpu()


CASES = [(torch.float32, 32), (torch.float32, 64), (torch.float32, 96), (torch.float32, 128),
         (torch.float16, 32), (torch.float16, 64), (torch.float16, 128)]


@pytest.mark.parametrize("ci", range(5), ids=lambda i: f"ctx{i}")
@pytest.mark.parametrize("arith", [1, 0], ids=["arith", "table"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("pdtype,dh", CASES, ids=lambda x: _ID.get(x, str(x)))
def test_every_q_dimension_meets_its_own_k_dimension(pdtype, dh, T, arith, ci):
    from mgea import ops
    ctxs = _contexts(dh)
    totals = (ctxs[ci], ctxs[(ci + 2) % 5])                # the two rows see different contexts
    # T = 3: a row takes 3 new tokens when it sees at least 3, else 1; one row is always shorter than T (padded query rows)
    lens = None if T == 1 else [3 if n >= 3 else 1 for n in totals]
    if lens is not None and min(lens) == 3:
        lens[1] = 1
    ctx_len = [n - (1 if lens is None else lens[b]) for b, n in enumerate(totals)]
    rows = np.ones((B, T), dtype=bool) if lens is None else np.arange(T)[None, :] < np.asarray(lens)[:, None]
    k, v, valid = _keys(totals, dh)
    image, table, ab = _page_setup(B, H, dh, pdtype, arith, seed=dh + ci)
    ops.kv_pages_write(image, torch.from_numpy(k).to(pdtype), torch.from_numpy(v).to(pdtype), table, valid=valid)
    image, table_d = image.cuda(), torch.from_numpy(table).cuda()
    cl = torch.tensor(ctx_len).cuda()
    ln = None if lens is None else torch.tensor(lens).cuda()
    one_split = np.asarray(totals) <= 4 * 64               # every page of the row belongs to split 0
    for dims in _rounds(T, dh):
        q = _queries(dims, dh)
        exp = _closed_form(dims, v, valid, dh)
        err = float(np.abs(_ref64(q, k, v, valid) - exp).max())
        assert err < 1e-6, f"the closed form is {err:.2e} off fp64 softmax attention: the inputs do not isolate the dimension"
        outs = {}
        for split in ([False, True] if T == 1 else [False]):
            out = _launch(q, image, table_d, ab, cl, ln, split, T)
            outs[split] = out
            got = out.double().numpy().reshape(exp.shape)
            bad = ~(np.abs(got - exp) <= TOL) & rows[:, :, None, None]
            if bad.any():
                b, i, h, d = (int(x[0]) for x in np.nonzero(bad))
                raise AssertionError(f"dh={dh} T={T} totals={totals} split={split} arith={arith}: {int(bad.sum())} wrong outputs; first at "
                                     f"row {b} query {i} head {h} (q dimension {int(dims[b, i, h])}) dim {d}: got {got[b, i, h, d]!r}, "
                                     f"expected {exp[b, i, h, d]!r}")
            if not rows.all():
                assert float(out[torch.from_numpy(~rows)].abs().max()) == 0.0, "a padded query row is not zero"
        if T == 1 and pdtype == torch.float32:
            for b in np.nonzero(one_split)[0]:
                assert torch.equal(outs[True][b], outs[False][b]), f"row {b} ({totals[b]} tokens): split and plain grid differ in bits"
