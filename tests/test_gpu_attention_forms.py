"""The forms of the fp32 dense attention (csrc/attn_dense.hip) and of the paged attention (csrc/attn_paged.hip) that the engines launch
and no test reached, on the closed-form input families of tests/test_gpu_attention_exact.py (pointer, poison, histogram: one lost,
doubled or wrongly admitted key moves an output by O(1)).

  dense   head_dim 32 / 64 / 96, H = 3, B = 4; an arbitrary key mask whose first 64-key tile holds no valid key (the `msafe` branch),
          mask and lens together, packed rows (cu), the k-tiled output layout, a canary behind and between everything that is written,
          a row without a valid key (zeros), the refusals;
  paged   layer > 0 of a several-layer pool, the k-tiled output, ONE split scratch across launches (counters left zero, stale partials
          never merged), 2 / 3 / 16 splits, and the split kernel's page loop past its first iteration (contexts over 2048 tokens at
          B * H = 64).

Every tolerance is ULP[torch.float32] (the project's 2e-5: absolute for pointer and poison, relative for histogram) or 2e-5 against
fp64 for the one diffuse case; every other comparison is bitwise.  The premises (every Case builds, the tiled_off restatement, the
split rule, the masks) are proved on the CPU in tests/test_attention_forms_host.py."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_attention_exact as AX
from test_gpu_attention_exact import FAMILIES, ULP, Case, _ID, _packed_case, _paged_cases, _ref64

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _bits(t):
    """the same bits as int32 (a poison NaN compares equal to itself)"""
    return t.detach().cpu().contiguous().view(torch.int32)


def _poison_bits():
    from mgea import ops
    return int(ops.POISON_BITS)


# ---- the k-tiled activation layout, restated (csrc/common.h tiled_off) --------------------------------------------------------
def tiled_off(row, n, N):
    """float offset of element (row, n) of a k-tiled [M, N] buffer: 64-row groups of 64 * N floats, 32-wide k-chunks of 2048 floats,
    inside a chunk the 16-byte group of (row, k .. k + 3) at [row / 16][(k / 4) % 2][(k / 8) % 4 * 16 + row % 16]"""
    row, n = np.asarray(row, dtype=np.int64), np.asarray(n, dtype=np.int64)
    r = row & 63
    return (row >> 6) * 64 * N + (n >> 5) * 2048 + ((((r >> 4) * 2 + ((n >> 2) & 1)) * 64 + ((n >> 3) & 3) * 16 + (r & 15)) << 2) + (n & 3)


def tiled_map(M, N):
    """[M, N] int64: where every element of a row-major [M, N] matrix lives in the tiled buffer"""
    return tiled_off(np.arange(M)[:, None], np.arange(N)[None, :], N)


def _check_tiled(tiled, rowmajor, M, N, what):
    """tiled: the flat buffer a kernel wrote over poison; rowmajor [M, N]: the same launch with a row-major out.  Both readings of the
    tiled buffer -- ops.untile_rows and the numpy restatement -- equal the row-major run bit for bit, and every float no row of M maps
    to is still poison."""
    from mgea import ops
    want = _bits(rowmajor.reshape(M, N))
    assert torch.equal(_bits(ops.untile_rows(tiled, M, N)), want), f"{what}: untile_rows(tiled out) differs from the row-major run"
    off = tiled_map(M, N)
    flat = _bits(tiled).numpy()
    assert flat.size == ops.tiled_floats(M, N)
    assert np.array_equal(flat[off], want.numpy()), f"{what}: the tiled out read through tiled_off differs from the row-major run"
    untouched = np.ones(flat.size, dtype=bool)
    untouched[off.ravel()] = False
    bad = np.nonzero(untouched & (flat != _poison_bits()))[0]
    assert bad.size == 0, f"{what}: {bad.size} floats that no row maps to were written, first at offset {int(bad[0])}"


# ---- dense fp32: shapes and masks ---------------------------------------------------------------------------------------------
D_B, D_H = 4, 3                      # H = 3: the head offset h * head_dim is no power of two
D_DH = (32, 64, 96)
D_T = (1, 63, 64, 65, 127, 128, 129, 300)   # a 64-query block / 64-key tile: partial, exact fit, a next tile holding a single key
D_KINDS = ("none", "prefix_lens", "prefix_mask", "random", "both")


def _prefix_lens(B, T):
    return np.asarray([(T, 1, min(64, T), max(1, T - 1), max(1, T // 2), T, min(2, T), max(1, T - 63))[b % 8] for b in range(B)])


def _random_mask(T, seed):
    """[D_B, T] bool, built like _cls_valid.  T > 64: row 0 has the kernel's whole first 64-key tile masked and its first valid key
    at 64 (the `mnew == -inf` -> msafe = 0 path, then alpha = 0 from mx == -inf), row 1 has key 0 masked, row 2 a single valid key (the
    last), row 3 is plain random; T <= 64 has no second tile: key 0 valid in every row, row 2 keeps a single key."""
    m = np.random.RandomState(seed + T).rand(D_B, T) > 0.3
    if T > 64:
        m[0, :64] = False
        m[0, 64] = True
        m[1, 0] = False
        m[1, 1] = True
        m[2, :] = False
        m[2, T - 1] = True
        m[3, 0] = True
    else:
        m[:, 0] = True
        m[2, 1:] = False
    return m


def dense_valid(kind, T):
    """-> (valid [D_B, T] bool, lens [D_B] or None, mask [D_B, T] bool or None): what the kernel is handed and the key set it must use"""
    ar = np.arange(T)[None, :]
    if kind == "none":
        return np.ones((D_B, T), dtype=bool), None, None
    if kind in ("prefix_lens", "prefix_mask"):
        lens = _prefix_lens(D_B, T)
        valid = ar < lens[:, None]
        return (valid, lens, None) if kind == "prefix_lens" else (valid, None, valid.copy())
    if kind == "random":
        m = _random_mask(T, 3000)
        return m, None, m.copy()
    assert kind == "both"
    # a random mask and a lens that cuts it: the valid set is the intersection.  Row 3 (T > 64): the mask leaves only keys >= 64 and
    # lens = 65 leaves only key 64 of those; row 1 loses its key 0 to the mask and its tail to lens.
    m = np.random.RandomState(4000 + T).rand(D_B, T) > 0.3
    lens = np.asarray([max(1, T - 3), max(2, T // 2) if T > 1 else 1, T, min(T, 65)])
    m[:, 0] = True
    if T > 64:
        m[1, 0] = False
        m[1, 1] = True
        m[3, :64] = False
        m[3, 64] = True
    return m & (ar < lens[:, None]), lens, m


@functools.lru_cache(maxsize=None)
def dense_case(family, kind, T, dh):
    return Case(family, dense_valid(kind, T)[0], D_H, dh)


def dense_case_list():
    """every (family, kind, T, head_dim) of the dense grid (tests/test_attention_forms_host.py builds them all on the CPU)"""
    return [(f, kind, T, dh) for dh in D_DH for kind in D_KINDS for T in D_T for f in FAMILIES]


def _i32(x):
    return None if x is None else torch.from_numpy(np.asarray(x)).to(torch.int32).cuda()


def _dense_run(qkv, H, lens=None, mask=None, cu=None, tiled=False, what=""):
    """one launch into a poisoned out with a guard row behind it -> the out (guard cut off).  Every float of a real query row is written
    (a padded query row t >= lens[b] is written too: today's behaviour; nothing reads it and its values are not checked) and the guard
    row is untouched."""
    from mgea import ops
    rows = qkv.shape[0] if cu is not None else qkv.shape[0] * qkv.shape[1]
    C = qkv.shape[-1] // 3
    n = ops.tiled_floats(rows, C) if tiled else rows * C
    buf = ops.poison(n + C, device="cuda")
    ops.attention(qkv.cuda(), H, lens=_i32(lens), mask=_i32(mask), cu=_i32(cu), tiled=tiled, out=buf)
    b = _bits(buf).numpy()
    assert (b[n:] == _poison_bits()).all(), f"{what}: the guard row behind out was written"
    if not tiled:
        assert (b[:n] != _poison_bits()).all(), f"{what}: {int((b[:n] == _poison_bits()).sum())} floats of real query rows were not written"
    return buf[:n]


def _real_rows(lens, B, T):
    """[B, T] bool: the query rows whose values are checked -- under lens the padded rows t >= lens[b] are written by the kernel (see
    _dense_run) but nothing reads them"""
    return None if lens is None else np.arange(T)[None, :] < np.asarray(lens)[:, None]


@pytest.mark.parametrize("kind", D_KINDS)
@pytest.mark.parametrize("dh", D_DH)
def test_attention_f32_every_head_dim_and_mask_counts_every_valid_key_exactly_once(dh, kind):
    """attn_dense_kernel<32 / 64 / 96> off the grid's origin (H = 3, B = 4) under no mask, a prefix as lens and as mask, an arbitrary
    mask whose first tile is empty, and mask + lens together."""
    for T in D_T:
        valid, lens, mask = dense_valid(kind, T)
        for family in FAMILIES:
            case = dense_case(family, kind, T, dh)
            what = f"fp32 dense dh={dh} T={T} {kind}"
            out = _dense_run(case.qkv(), D_H, lens=lens, mask=mask, what=what)
            case.check(out.view(D_B, T, -1), F32, rows=_real_rows(lens, D_B, T), what=what)


D_PACKED = {32: (1, 20, 64, 65), 64: (1, 20, 64, 65, 129), 96: (1, 20, 64, 65, 129)}   # poison: 8 dims per sequence, 8 * 5 > 32


@pytest.mark.parametrize("dh", D_DH)
def test_attention_f32_packed_rows_stay_inside_their_sequence(dh):
    """cu_seqlens input (DistilBERT on unpadded batches in the f32 engine): the grid is sized for the longest sequence, a block past a
    sequence's end leaves at once and the key loop stops at the sequence's own length; poison: the keys of the other sequences are loud."""
    seqs = D_PACKED[dh]
    cu = np.concatenate([[0], np.cumsum(seqs)])
    for family in FAMILIES:
        qkv, exp = _packed_case(family, seqs, D_H, dh)
        out = _dense_run(qkv, D_H, cu=cu, what=f"packed {family} dh={dh}")
        got = out.double().cpu().numpy().reshape(exp.shape)
        tol = ULP[F32] * (exp if family == "histogram" else 1.0)
        bad = ~(np.abs(got - exp) <= tol)
        assert not bad.any(), (f"{family} dh={dh}: {int(bad.sum())} wrong outputs, first at packed row {int(np.nonzero(bad)[1][0])}: "
                               f"got {got[bad][0]!r}, expected {exp[bad][0]!r}")


D_TILED = ((1, 64), (3, 70), (8, 64), (2, 200))     # M = B * T <= 512; (3, 70): a batch row across a 64-row group boundary; (2, 200): a partial last group


def tiled_lens(B, T):
    """the decoder passes lens for a batch of ragged prompts: every shape but the single row"""
    return None if B == 1 else _prefix_lens(B, T)


@functools.lru_cache(maxsize=None)
def tiled_case(family, B, T, dh):
    lens = tiled_lens(B, T)
    valid = np.ones((B, T), dtype=bool) if lens is None else np.arange(T)[None, :] < lens[:, None]
    return Case(family, valid, D_H, dh)


@pytest.mark.parametrize("B,T", D_TILED)
@pytest.mark.parametrize("dh", D_DH)
def test_attention_f32_tiled_output_is_the_row_major_output_in_another_place(dh, B, T):
    """tiled_out = 1, the output layout of every fused prefill of up to 512 rows"""
    lens = tiled_lens(B, T)
    M, C = B * T, D_H * dh
    for family in FAMILIES:
        case = tiled_case(family, B, T, dh)
        what = f"fp32 dense tiled dh={dh} B={B} T={T} {family}"
        plain = _dense_run(case.qkv(), D_H, lens=lens, what=what)
        case.check(plain.view(B, T, C), F32, rows=_real_rows(lens, B, T), what=what + " (row-major)")
        tiled = _dense_run(case.qkv(), D_H, lens=lens, tiled=True, what=what)
        _check_tiled(tiled, plain, M, C, what)


def test_attention_f32_diffuse_softmax_against_fp64():
    """Uniform +-1.5 inputs (the distribution of test_attention_dense and CLS_DIFFUSE_BOUND) at head_dim 96, T = 300 under the random
    mask (row 0: empty first tile, row 2: one key), against fp64; bound: the project's 2e-5.  Observed on MI355X: 2.5e-7"""
    B, T, H, dh = D_B, 300, D_H, 96
    g = torch.Generator().manual_seed(96300)
    qkv = (torch.rand(B, T, 3 * H * dh, generator=g) * 2 - 1) * 1.5
    valid, _, mask = dense_valid("random", T)
    q, k, v = (qkv[..., i * H * dh:(i + 1) * H * dh].reshape(B, T, H, dh).double().numpy() for i in range(3))
    want = _ref64(q, k, v, valid).reshape(B, T, H * dh)
    got = _dense_run(qkv, H, mask=mask, what="diffuse").view(B, T, -1).double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"[attention f32 diffuse] dh={dh} T={T} random mask: max |out - fp64| = {err:.3e} (bound {AX.CLS_DIFFUSE_BOUND:.1e})")
    assert err < AX.CLS_DIFFUSE_BOUND


NO_KEY_S = (1, 65, 300)


def no_key_inputs(S, how):
    """-> (lens, mask) under which row 1 of D_B rows has no valid key and every other row has all of them"""
    if how == "mask":
        m = np.ones((D_B, S), dtype=bool)
        m[1] = False
        return None, m
    return np.asarray([S, 0, S, S]), None


@pytest.mark.parametrize("how", ["mask", "lens"])
@pytest.mark.parametrize("dh", D_DH)
def test_attention_f32_row_without_a_valid_key_gives_zeros(dh, how):
    """The kernel's contract (_ref64 cannot express it), the same as attn_cls.hip's: a row whose every key is masked (or lens = 0) gives
    all-zero, finite output rows -- the sum of p is 0 and the kernel selects 0 instead of 1 / 0; its neighbours are untouched by it.
    Before the select: 0 * inf = NaN in every float of that row."""
    for S in NO_KEY_S:
        case = Case("poison", np.ones((D_B, S), dtype=bool), D_H, dh)
        lens, mask = no_key_inputs(S, how)
        out = _dense_run(case.qkv(), D_H, lens=lens, mask=mask, what=f"S={S} row 1 without a key").view(D_B, S, -1).cpu()
        assert torch.equal(out[1], torch.zeros_like(out[1])), f"dh={dh} S={S} ({how}): the row without a valid key is not zero: {out[1].flatten()[:4].tolist()}"
        rows = np.ones((D_B, S), dtype=bool)
        rows[1] = False
        case.check(out, F32, rows=rows, what=f"dh={dh} S={S}, row 1 fully masked ({how})")


def test_attention_f32_refusals():
    from mgea import ops
    qkv = torch.zeros(2, 4, 3 * 2 * 128).cuda()
    with pytest.raises(RuntimeError, match="not supported"):
        ops.attention(qkv, 2)                               # head_dim 128
    qkv = torch.zeros(8, 3 * 2 * 64).cuda()
    cu = torch.tensor([0, 4, 8]).cuda()
    assert ops.attention(qkv, 2, cu=cu).shape == (8, 128)   # the shape itself is fine
    with pytest.raises(RuntimeError, match="packed rows carry no"):
        ops.attention(qkv, 2, cu=cu, mask=torch.ones(2, 4, dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError, match="packed rows carry no"):
        ops.attention(qkv, 2, cu=cu, lens=torch.tensor([4, 4]).cuda())
    with pytest.raises(RuntimeError, match="packed rows carry no"):
        ops.attention(qkv, 2, cu=cu, tiled=True)


# ---- the paged attention --------------------------------------------------------------------------------------------------------
P_H = 2
P_FORMS = [(torch.float32, 64), (torch.float32, 96), (torch.float16, 64)]
P_TILED_FORMS = [(torch.float32, 32), (torch.float32, 64), (torch.float32, 96), (torch.float16, 64)]
_form_id = lambda x: _ID.get(x, str(x))      # noqa: E731


def split_rule(B, H, T, max_pages, limit=64):
    """attn_split_count (csrc/attn_paged.hip) restated: workgroups per (row, head, query) of a launch that has a split scratch.  Only
    the decode step's single query, only while B * H is within the switch attn_split (default 64) and the scratch's 256 items, only
    with more than one wave-round of pages; then one split per 4 table pages, at most 512 / (B * H) (two workgroups per CU), at most 16."""
    if limit <= 0 or T != 1 or B * H > limit or B * H > 256 or max_pages <= 4:
        return 1
    return max(1, min((max_pages + 3) // 4, 512 // (B * H), 16))


def page_table(B, width, arith, seed):
    """-> (table [B, width], pages per layer, arith_batch): computed ids j * B + b, or a random permutation into a pool with 8 pages
    nobody owns"""
    if arith:
        return np.arange(width)[None, :] * B + np.arange(B)[:, None], width * B, B
    n_pages = width * B + 8
    return np.random.RandomState(seed).permutation(n_pages)[:B * width].reshape(B, width), n_pages, 0


def page_image(case, pdtype, table, n_pages, n_layer=1, layer=0):
    """n_layer layers of pages, every slot poison (K 8, V 1024: the poison of _page_setup), the case's valid keys written into `layer`"""
    from mgea import ops
    per = ops.kv_page_elems(n_pages, case.H, case.dh)
    image = torch.empty(n_layer * per, dtype=pdtype)
    img = image.view(n_layer * n_pages, 2, -1)
    img[:, 0] = 8.0
    img[:, 1] = 1024.0
    k, v = (torch.from_numpy(x).to(pdtype) for x in (case.k, case.v))
    ops.kv_pages_write(image.view(n_layer, per)[layer], k, v, table, valid=case.valid)
    return image


def _q_rows(case):
    """qkv [B, Tq, 3C] whose K | V columns are NaN: the kernel reads K | V from the pages only"""
    B, Tq = case.q.shape[:2]
    C = case.H * case.dh
    qkv = torch.full((B, Tq, 3 * C), float("nan"))
    qkv[..., :C] = torch.from_numpy(case.q.reshape(B, Tq, C)).float()
    return qkv.cuda()


def _paged_launch(case, pages, table, n_pages, ab, ctx_len, lens=None, split=True, layer=0, n_layer=1, tiled=False, scratch=None, info=None,
                  what=""):
    """one launch into a poisoned out with a guard row behind it -> out (guard cut off; row-major: [B, Tq, C])"""
    from mgea import ops
    B, Tq = case.q.shape[:2]
    C = case.H * case.dh
    n = ops.tiled_floats(B * Tq, C) if tiled else B * Tq * C
    buf = ops.poison(n + C, device="cuda")
    ops.attention_paged(_q_rows(case), case.H, pages, torch.from_numpy(table).cuda(), torch.tensor(ctx_len).cuda(),
                        None if lens is None else torch.tensor(lens).cuda(), arith_batch=ab, split=split, info=info, layer=layer,
                        n_layer=n_layer, tiled=tiled, out=buf, scratch=scratch)
    b = _bits(buf).numpy()
    assert (b[n:] == _poison_bits()).all(), f"{what}: the guard row behind out was written"
    if not tiled:
        assert (b[:n] != _poison_bits()).all(), f"{what}: {int((b[:n] == _poison_bits()).sum())} floats of out were not written"
        return buf[:n].view(B, Tq, C)
    return buf[:n]


P_LAYER_CTX = [(65, 257), (1000, 1)]


@pytest.mark.parametrize("ctx", P_LAYER_CTX, ids=lambda c: f"ctx{c[0]}_{c[1]}")
@pytest.mark.parametrize("arith", [1, 0], ids=["arith", "table"])
@pytest.mark.parametrize("split", [0, 1], ids=["one_wg", "split"])
@pytest.mark.parametrize("pdtype,dh", P_FORMS, ids=_form_id)
def test_attention_paged_reads_the_layer_it_is_given(pdtype, dh, split, arith, ctx):
    """A pool of 3 layers, launched at layer 1 and at layer 2: `lbase = base + layer * layer_stride * EB` with a non-zero layer term.
    The pages of the other layers hold poison (K 8, V 1024), so a wrong layer gives 1024."""
    table, n_pages, ab = page_table(2, AX.MAX_PAGES, arith, seed=dh + ctx[0])
    for layer in (1, 2):
        for family in FAMILIES:
            cases = _paged_cases(family, ctx, 1, P_H, dh)
            pages = page_image(cases[0], pdtype, table, n_pages, n_layer=3, layer=layer).cuda()       # K | V are the same in every round
            for case in cases:
                info, what = [], f"paged layer {layer} of 3, dh={dh} ctx={ctx} split={split} arith={arith}"
                out = _paged_launch(case, pages, table, n_pages, ab, [c - 1 for c in ctx], split=bool(split), layer=layer, n_layer=3, info=info,
                                    what=what)
                assert info == [4 if split else 1], f"workgroups per query: {info}"
                case.check(out, F32, what=what)


P_TILED_CTX = {2: (65, 257), 5: (1, 64, 65, 257, 1000)}


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("split", [0, 1], ids=["one_wg", "split"])
@pytest.mark.parametrize("pdtype,dh", P_TILED_FORMS, ids=_form_id)
def test_attention_paged_tiled_output_decode(pdtype, dh, split, B):
    """tiled_out = 1 at T = 1, what every fused decode step launches: the same floats as the row-major run at their tiled addresses,
    everything else in the 64-row group untouched"""
    ctx = P_TILED_CTX[B]
    table, n_pages, ab = page_table(B, AX.MAX_PAGES, 1, seed=dh)
    for family in FAMILIES:
        cases = _paged_cases(family, ctx, 1, P_H, dh)
        pages = page_image(cases[0], pdtype, table, n_pages).cuda()
        for case in cases:
            what = f"paged tiled decode dh={dh} B={B} split={split} {family}"
            kw = dict(ctx_len=[c - 1 for c in ctx], split=bool(split), what=what)
            plain = _paged_launch(case, pages, table, n_pages, ab, **kw)
            case.check(plain, F32, what=what + " (row-major)")
            tiled = _paged_launch(case, pages, table, n_pages, ab, tiled=True, **kw)
            _check_tiled(tiled, plain, B, P_H * dh, what)


@pytest.mark.parametrize("pdtype,dh", P_TILED_FORMS, ids=_form_id)
def test_attention_paged_tiled_output_ragged_extend(pdtype, dh):
    """The extend form of test_attention_paged_ragged_extend (T = 3 new tokens, lens = [3, 1]) with tiled_out = 1: the zero rows of the
    two padded queries land at their tiled addresses"""
    ctx_len, lens = [62, 130], [3, 1]
    total = tuple(c + n for c, n in zip(ctx_len, lens))
    rows = np.arange(3)[None, :] < np.asarray(lens)[:, None]
    table, n_pages, ab = page_table(2, AX.MAX_PAGES, 0, seed=dh)
    C = P_H * dh
    for family in FAMILIES:
        cases = _paged_cases(family, total, 3, P_H, dh)
        pages = page_image(cases[0], pdtype, table, n_pages).cuda()
        for case in cases:
            what = f"paged tiled extend dh={dh} {family}"
            plain = _paged_launch(case, pages, table, n_pages, ab, ctx_len, lens=lens, what=what)
            case.check(plain, F32, rows=rows, what=what + " (row-major)")
            assert float(plain[1, 1:].abs().max()) == 0.0
            tiled = _paged_launch(case, pages, table, n_pages, ab, ctx_len, lens=lens, tiled=True, what=what)
            _check_tiled(tiled, plain, 6, C, what)
            flat = tiled.cpu().numpy()
            assert (flat[tiled_map(6, C)[4:6]] == 0.0).all(), "the padded queries' zero rows are not at their tiled addresses"


# active splits of a row at 4 launched: min(4, ceil(pages / 4)) -- 1000 tokens: 16 pages -> 4; 400: 7 pages -> 2; 65 and 1: -> 1
P_REUSE = [((1000, 65), (4, 1)), ((400, 1000), (2, 4)), ((65, 1), (1, 1)), ((1000, 769), (4, 4))]


def active_splits(ctx, nsplit):
    return min(nsplit, ((ctx + 63) // 64 + 3) // 4)


@pytest.mark.parametrize("pdtype,dh", P_FORMS, ids=_form_id)
def test_attention_paged_one_split_scratch_across_launches(pdtype, dh):
    """The kernel's contract for its scratch (csrc/common.h): the counters are zeroed ONCE and every launch leaves them zero; a partial
    that an earlier launch left is never merged.  One caller scratch -- part starts as poison -- serves launches whose rows need (4, 1),
    (2, 4), (1, 1) and (4, 4) active splits of 4 launched, every family, every pointer round; part is poisoned again in front of the
    (1, 1) launches, which may not read it.  Each launch: exact, bitwise equal to the same launch on a scratch of its own, counters zero."""
    from mgea import ops
    table, n_pages, ab = page_table(2, AX.MAX_PAGES, 0, seed=dh + 5)
    part, count = ops.attn_split_scratch(dh)
    for family in FAMILIES:
        for i, (ctx, active) in enumerate(P_REUSE):
            assert tuple(active_splits(c, 4) for c in ctx) == active
            if i == 2:
                part.copy_(ops.poison(part.numel(), device="cuda").view_as(part))
            cases = _paged_cases(family, ctx, 1, P_H, dh)
            pages = page_image(cases[0], pdtype, table, n_pages).cuda()
            for case in cases:
                info, what = [], f"paged scratch reuse dh={dh} {family} launch {i + 1} ctx={ctx}"
                out = _paged_launch(case, pages, table, n_pages, ab, [c - 1 for c in ctx], scratch=(part, count), info=info, what=what)
                assert info == [4], f"{what}: workgroups per query {info}"       # max_pages = 16: the split form, whatever the contexts
                assert not bool(count.any()), f"{what}: counters left non-zero: {count.nonzero().flatten().tolist()}"
                case.check(out, F32, what=what)
                fresh = _paged_launch(case, pages, table, n_pages, ab, [c - 1 for c in ctx], what=what + " (own scratch)")
                assert torch.equal(_bits(out), _bits(fresh)), f"{what}: differs from the same launch on a fresh scratch"


# (table width, contexts, pointer index bits): B * H = 4
P_WIDTHS = [(8, (257, 512), 10), (9, (513, 576), 10), (64, (4096, 3841), 12), (64, (65, 1), 10)]


@pytest.mark.parametrize("width,ctx,nbits", P_WIDTHS, ids=lambda x: "_".join(map(str, x)) if isinstance(x, tuple) else str(x))
@pytest.mark.parametrize("pdtype,dh", P_FORMS, ids=_form_id)
def test_attention_paged_split_counts_from_the_table_width(pdtype, dh, width, ctx, nbits):
    """2, 3 and 16 workgroups per query (the merge is unrolled over 16): 8 wide -> 2; 9 wide -> 3, the second row exactly fills its last
    page; 64 wide -> 16, all active with the edge of the sixteenth (4096 and 3841 tokens), and 16 launched with one active."""
    from mgea import ops
    table, n_pages, ab = page_table(2, width, width % 2, seed=dh + width)
    want = split_rule(2, P_H, 1, width)
    assert want == {8: 2, 9: 3, 64: 16}[width] and ops.attn_split_count(2, P_H, 1, width) == want
    for family in FAMILIES:
        cases = _paged_cases(family, ctx, 1, P_H, dh, nbits)
        pages = page_image(cases[0], pdtype, table, n_pages).cuda()
        for case in cases:
            info, what = [], f"paged width {width} dh={dh} ctx={ctx} {family}"
            out = _paged_launch(case, pages, table, n_pages, ab, [c - 1 for c in ctx], info=info, what=what)
            assert info == [want], f"{what}: workgroups per query {info}, the rule says {want}"
            case.check(out, F32, what=what)


LOOP_B, LOOP_H, LOOP_DH, LOOP_WIDTH = 8, 8, 32, 40
LOOP_CTX = (2049, 2112, 2113, 1, 64, 2050, 513, 2100)


def loop_cases(family):
    """one round at a time, nothing kept: a round of this shape holds 70 MB of fp64 K | V"""
    return AX._paged_case_iter(family, LOOP_CTX, 1, LOOP_H, LOOP_DH, 12)


@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=_ID.get)
def test_attention_paged_split_loop_past_its_first_iteration(pdtype):
    """B * H = 64 on a table 40 wide: room = 512 / 64 caps the launch at 8 splits, pg_step = 32, and rows 0, 1, 2, 5 and 7 (more than
    2048 tokens) send split 0 round its page loop a second time -- `pg += pg_step` with the next K requested under PV.  Rows 0 and 5
    leave one or two tokens on page 32, row 7 a partial page 32 for waves 0 .. 3 (2100 = 32 * 64 + 52).  The image is the 320 pages
    the table names, nothing more."""
    from mgea import ops
    B, H, dh = LOOP_B, LOOP_H, LOOP_DH
    arith = pdtype == torch.float16                           # computed page ids for one dtype, a permutation for the other
    if arith:
        table, n_pages, ab = page_table(B, LOOP_WIDTH, 1, 0)
    else:
        table, n_pages, ab = np.random.RandomState(40).permutation(B * LOOP_WIDTH).reshape(B, LOOP_WIDTH), B * LOOP_WIDTH, 0
    assert n_pages == 320
    want = split_rule(B, H, 1, LOOP_WIDTH)
    assert want == 8 and ops.attn_split_count(B, H, 1, LOOP_WIDTH) == 8
    for family in FAMILIES:
        pages = None
        for case in loop_cases(family):
            if pages is None:                                     # K | V are the same in every round
                pages = page_image(case, pdtype, table, n_pages).cuda()
            info, what = [], f"paged split loop {_ID[pdtype]} {family}"
            out = _paged_launch(case, pages, table, n_pages, ab, [c - 1 for c in LOOP_CTX], info=info, what=what)
            assert info == [8], f"{what}: workgroups per query {info}"
            case.check(out, F32, what=what)
