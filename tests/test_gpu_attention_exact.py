"""Attention kernels on inputs whose exact answer is known in closed form.

Random qkv with a spread-out softmax tests "roughly right": one key of 1024 is worth 1.5e-3 of the output, below every 16-bit bound.
Here a wrong SET of participating keys -- one lost at a tile, stage or page boundary, a padding key counted, a key read twice after
an index clamp -- moves the output by O(1):

  pointer    key t carries its index as a +-1 code over the head dimensions, query i is beta * code(pi(i)): the softmax is a
             one-hot of key pi(i) (the next key is e^-20 away) and out[i] = V[pi(i)], where pi visits the keys at which kernels
             break: 0, 31, 32, 63, 64, both ends of every 64-key tile and every 128- / 256-key stage, T - 1, the neighbours of masked
             keys and the last valid key of a ragged row;
  poison     valid keys have K = 0 and V = 1, every invalid key (masked, at or past lens[b], the unused slots of a KV page) has
             V = 1024 and a K aligned with q: out = 1 exactly unless an invalid key is counted, then ~1024;
  histogram  q = 0 and V[t] = e_(t mod dh): out[d] * n_valid = the number of valid keys with t mod dh = d; a key dropped or counted
             twice moves a bin by 1 / count >= 1 / 16.

All q, k, v values are exact in bf16 AND fp16, so the same inputs serve every kernel, and for every input the closed form is held
to fp64 softmax attention on the CPU (1e-6): that assertion is the condition on the inputs.  The tolerance is one ulp of the
output type at 1.0 (absolute for pointer and poison, relative for histogram): 2^-7 bf16, 2^-10 fp16, 2e-5 for fp32 outputs."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2e-5}
NBITS = 10                       # index bits of the pointer code: keys 0 .. 1023
FAMILIES = ("pointer", "poison", "histogram")


# ---- the input families (host, fp64 holding 16-bit-exact values) --------------------------------------------------------------
def _code(idx, dh, nbits=NBITS):
    """+-1 code of the key index: bit j on dims j r .. j r + r - 1, r = dh // nbits; the remaining dims are 0"""
    r = dh // nbits
    bits = ((np.asarray(idx)[..., None] >> np.arange(nbits)) & 1) * 2 - 1
    out = np.zeros(np.asarray(idx).shape + (dh,))
    out[..., :nbits * r] = np.repeat(bits, r, axis=-1)
    return out


def _beta(dh, nbits=NBITS):
    """smallest power of two with a scaled score gap 2 r beta / sqrt(dh) >= 20 between key pi(i) and any other key"""
    r = dh // nbits
    return 2.0 ** math.ceil(math.log2(20.0 * math.sqrt(dh) / (2 * r)))


def _targets(valid_b, extra=()):
    """the keys of one row at which kernels break (valid ones only), in a fixed order"""
    T = len(valid_b)
    cand = [0, 31, 32, 63, 64, T - 1, *extra]
    for step in (64, 128, 256):
        for j in range(0, T, step):
            cand += [j, j + step - 1]
    inv = np.nonzero(~valid_b)[0]
    cand += [*(inv - 1), *(inv + 1)] if len(inv) <= T // 2 else []        # the neighbours of masked keys
    nz = np.nonzero(valid_b)[0]
    cand += [int(nz[-1]), int(nz[0])]
    seen, out = set(), []
    for t in cand:
        t = int(t)
        if 0 <= t < T and valid_b[t] and t not in seen:
            seen.add(t)
            out.append(t)
    return out


def _v_rows(B, T, H, dh, b0=0):
    """multiples of 1/8 in [-2, 2] that differ between neighbouring keys, heads and rows"""
    b, t, h, d = np.meshgrid(np.arange(B) + b0, np.arange(T), np.arange(H), np.arange(dh), indexing="ij")
    return ((7 * t + 3 * d + 5 * h + 11 * b) % 33 - 16) / 8.0


def _family(family, valid, H, dh, Tq=None, b0=0, q_targets=None, nbits=NBITS):
    """-> q [B, Tq, H, dh], k, v [B, T, H, dh], expected [B, Tq, H, dh] (fp64 arrays).  valid [B, T] bool; Tq queries per row (None: T).
    q_targets[b][h][i] (pointer only): the key query (b, h, i) points at; None: cycle through _targets().
    nbits: index bits of the pointer code (rows of up to 2^nbits keys); the default keeps every earlier case bit-identical."""
    B, T = valid.shape
    assert T <= 2 ** nbits, f"{T} keys need more than {nbits} index bits"
    Tq = T if Tq is None else Tq
    if family == "pointer":
        k = np.broadcast_to(_code(np.arange(T), dh, nbits)[None, :, None, :], (B, T, H, dh)).copy()
        v = _v_rows(B, T, H, dh, b0)
        pi = np.zeros((B, Tq, H), dtype=np.int64)
        for b in range(B):
            for h in range(H):
                if q_targets is not None:
                    pi[b, :, h] = q_targets[b][h]
                else:
                    L = _targets(valid[b])
                    pi[b, :, h] = [L[(i + 3 * h) % len(L)] for i in range(Tq)]
        assert all(valid[b, pi[b]].all() for b in range(B))
        q = _beta(dh, nbits) * _code(pi, dh, nbits)
        exp = np.stack([np.stack([v[b, pi[b, :, h], h] for h in range(H)], 1) for b in range(B)])
        return q, k, v, exp
    if family == "poison":
        q = np.zeros((B, Tq, H, dh))
        q[..., :8] = 8.0
        k = np.where(valid[:, :, None, None], 0.0, 8.0) * np.ones((1, 1, H, dh))
        v = np.where(valid[:, :, None, None], 1.0, 1024.0) * np.ones((1, 1, H, dh))
        return q, k, v, np.ones((B, Tq, H, dh))
    assert family == "histogram"
    q = np.zeros((B, Tq, H, dh))
    k = np.broadcast_to(_code(np.arange(T), dh, nbits)[None, :, None, :], (B, T, H, dh)).copy()
    v = np.zeros((B, T, H, dh))
    exp = np.zeros((B, Tq, H, dh))
    for b in range(B):
        for h in range(H):
            hot = (np.arange(T) + 3 * h + 5 * (b + b0)) % dh
            v[b, np.arange(T), h, hot] = 1.0
            cnt = np.bincount(hot[valid[b]], minlength=dh)
            exp[b, :, h] = cnt / valid[b].sum()
    return q, k, v, exp


def _ref64(q, k, v, valid):
    """plain fp64 softmax attention, one row at a time: [B, Tq, H, dh]"""
    out = np.empty(q.shape)
    for b in range(q.shape[0]):
        s = (q[b].transpose(1, 0, 2) @ k[b].transpose(1, 2, 0)) / math.sqrt(q.shape[-1])        # [H, Tq, T]
        s[:, :, ~valid[b]] = -np.inf
        p = np.exp(s - s.max(-1, keepdims=True))
        out[b] = ((p / p.sum(-1, keepdims=True)) @ v[b].transpose(1, 0, 2)).transpose(1, 0, 2)
    return out


def _exact16(x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return bool((t.bfloat16().double() == t).all()) and bool((t.half().double() == t).all())


class Case:
    def __init__(self, family, valid, H, dh, **kw):
        self.family, self.valid, self.H, self.dh = family, valid, H, dh
        self.q, self.k, self.v, self.exp = _family(family, valid, H, dh, **kw)
        assert _exact16(self.q) and _exact16(self.k) and _exact16(self.v), "inputs must be exact in bf16 and fp16"
        err = float(np.abs(_ref64(self.q, self.k, self.v, valid) - self.exp).max())
        assert err < 1e-6, f"{family}: the closed form is {err:.2e} off fp64 softmax attention: the inputs do not isolate the key set"

    def qkv(self):
        """dense [B, T, 3 C] fp32 (self-attention: as many queries as keys)"""
        B, T = self.valid.shape
        return torch.from_numpy(np.concatenate([x.reshape(B, T, -1) for x in (self.q, self.k, self.v)], -1)).float()

    def check(self, out, dtype, rows=None, what=""):
        """out [B, Tq, C] from a kernel whose output type is dtype; rows [B, Tq] bool: the query rows that are defined"""
        got = out.detach().double().cpu().numpy().reshape(self.exp.shape)
        exp, ulp = self.exp, ULP[dtype]
        tol = ulp * exp if self.family == "histogram" else np.full(exp.shape, ulp)
        bad = ~(np.abs(got - exp) <= tol)                                     # (a NaN is bad)
        if rows is not None:
            bad &= np.asarray(rows)[:, :, None, None]
        if bad.any():
            b, i, h, d = (int(x[0]) for x in np.nonzero(bad))
            raise AssertionError(f"{self.family} {what}: {int(bad.sum())} wrong outputs; first at row {b} query {i} head {h} dim {d}: "
                                 f"got {got[b, i, h, d]!r}, expected {exp[b, i, h, d]!r} +- {tol[b, i, h, d]:.2e}")


def _valid(kind, T):
    if kind == "none":
        return np.ones((2, T), dtype=bool)
    if kind == "prefix":
        lens = [T, 1, min(64, T), max(1, T - 1)]
        return np.arange(T)[None, :] < np.asarray(lens)[:, None]
    assert kind == "random"
    m = np.random.RandomState(1000 + T).rand(2, T) > 0.3
    m[:, 0] = True
    return m


@functools.lru_cache(maxsize=None)
def _dense_case(family, kind, T, H=2, dh=64):
    return Case(family, _valid(kind, T), H, dh)


# ---- the 16-bit flash attention ---------------------------------------------------------------------------------------------
T_LIST = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]
FORMS = [(0, 1), (2, 0), (2, 1)]                       # (attn16_wide, attn16_pipe): narrow, wide rolled, wide software-pipelined
DTYPES = [torch.bfloat16, torch.float16]
_ID = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


@pytest.mark.parametrize("T", T_LIST)
@pytest.mark.parametrize("kind", ["none", "prefix", "random"])
@pytest.mark.parametrize("wide,pipe", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_attention16_counts_every_valid_key_exactly_once(dtype, wide, pipe, kind, T, tune):
    from mgea import ops
    tune("attn16_wide", wide)
    tune("attn16_pipe", pipe)
    for family in FAMILIES:
        case = _dense_case(family, kind, T)
        mask = None if kind == "none" else torch.from_numpy(case.valid).to(torch.int32).cuda()
        out = ops.attention16(case.qkv().to(dtype).cuda(), case.H, mask=mask)
        case.check(out, dtype, what=f"T={T} {kind} mask, wide={wide} pipe={pipe}")


def _packed_case(family, seqs, H=2, dh=64):
    """the sequences back to back: q, k, v [1, n, H, dh] each; expected per sequence.  poison: the keys of the OTHER sequences are the
    invalid ones -- sequence s asks along its own 8 dims, its keys are loud along everybody else's, its V is 2^s: out = 2^s."""
    parts = []
    for s, n in enumerate(seqs):
        valid = np.ones((1, n), dtype=bool)
        if family == "poison":
            q = np.zeros((1, n, H, dh))
            q[..., 8 * s:8 * s + 8] = 8.0
            k = np.full((1, n, H, dh), 8.0)
            k[..., 8 * s:8 * s + 8] = 0.0
            v = np.full((1, n, H, dh), 2.0 ** s)
            exp = v.copy()
            assert _exact16(q) and _exact16(k) and _exact16(v)
            assert float(np.abs(_ref64(q, k, v, valid) - exp).max()) < 1e-6
        else:
            c = Case(family, valid, H, dh, b0=s)
            q, k, v, exp = c.q, c.k, c.v, c.exp
        parts.append((q, k, v, exp))
    q, k, v, exp = (np.concatenate([p[i] for p in parts], 1) for i in range(4))
    n = q.shape[1]
    return torch.from_numpy(np.concatenate([x.reshape(n, -1) for x in (q, k, v)], -1)).float(), exp


@pytest.mark.parametrize("seqs", [(1, 20, 128, 129, 256), (1, 20, 64, 65, 128)], ids=["to256_wide", "to128_narrow"])
@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_attention16_packed_rows_stay_inside_their_sequence(dtype, pipe, seqs, tune):
    """cu_seqlens input: the launcher takes the wide form when the longest sequence is over 128 tokens, the narrow form otherwise."""
    from mgea import ops
    tune("attn16_pipe", pipe)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(seqs)]), dtype=torch.int32)
    for family in FAMILIES:
        qkv, exp = _packed_case(family, seqs)
        got = ops.attention16(qkv.to(dtype).cuda(), 2, cu=cu.cuda()).double().cpu().numpy().reshape(exp.shape)
        tol = ULP[dtype] * (exp if family != "pointer" else 1.0)       # poison: out = 2^s, one ulp of THAT; histogram: relative
        bad = ~(np.abs(got - exp) <= tol)
        assert not bad.any(), f"{family}: {int(bad.sum())} wrong outputs, first at packed row {int(np.nonzero(bad)[1][0])}"


@functools.lru_cache(maxsize=None)
def _big_case(family):
    lens = np.asarray([1024, 1, 64, 1023, 513, 1024, 300, 129, 1000])
    return Case(family, np.arange(1024)[None, :] < lens[:, None], 8, 64)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_attention16_more_work_items_than_workgroups(dtype, tune):
    """B = 9, H = 8, T = 1024 on the narrow form: 576 (row, head, query block) items on 2 workgroups per CU -- the persistent loop moves
    on to a second item, with the output rows of the first held in registers across the hand-over."""
    from mgea import ops
    tune("attn16_wide", 0)
    for family in FAMILIES:
        case = _big_case(family)
        out = ops.attention16(case.qkv().to(dtype).cuda(), case.H, mask=torch.from_numpy(case.valid).to(torch.int32).cuda())
        case.check(out, dtype, what="B=9 H=8 T=1024")


# Diffuse softmax, the only case where the 16-bit rounding of P matters (the structured inputs above have P in {0, 1}): uniform +-1.5
# qkv at T = 1024 against fp64.  bf16 keeps the bound of tests/test_gpu_bf16.py (P rounded to 8 significand bits before P V); fp16 has
# three more significand bits: that bound / 8.  Observed on MI355X: bf16 5.5e-4, fp16 7.0e-5.
DIFFUSE_BOUND = {torch.bfloat16: 2.5e-2, torch.float16: 2.5e-2 / 8}


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_attention16_diffuse_softmax_against_fp64(dtype):
    from mgea import ops
    B, T, H, dh = 2, 1024, 2, 64
    g = torch.Generator().manual_seed(7)
    qkv = ((torch.rand(B, T, 3 * H * dh, generator=g) * 2 - 1) * 1.5).to(dtype)
    q, k, v = (qkv[..., i * H * dh:(i + 1) * H * dh].reshape(B, T, H, dh).double().numpy() for i in range(3))
    want = _ref64(q, k, v, np.ones((B, T), dtype=bool)).reshape(B, T, H * dh)
    got = ops.attention16(qkv.cuda(), H).double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"[attention16 diffuse] {_ID[dtype]} T={T}: max |out - fp64| = {err:.3e} (bound {DIFFUSE_BOUND[dtype]:.2e})")
    assert err < DIFFUSE_BOUND[dtype]


# ---- the fp16 window of the deferred rescale --------------------------------------------------------------------------------
def _rescale_window_inputs():
    """Search, in the kernel's own arithmetic, for 8-bit-significand (bf16- and fp16-exact) q = (qa, qb, 0, ...), k = (ka, kb, 0, ...)
    whose score sits in the window the old threshold left open: with the reference still at 0 (the first tile's keys are all zero),
    arg = fl32(s * kexp) <= 16 -- no rescale at RESCALE_LOG2 = 16 -- and p = 2^arg >= 65520, which fp16 rounds to +inf."""
    kexp = np.float32(0.125) * np.float32(1.4426950408889634)
    lo = 65520.0 * (1 + 2.0 ** -20)          # clear of the rounding boundary by more than the 1 ulp of v_exp_f32
    for qa, ka in ((8.0, 11.0), (4.0, 22.0), (16.0, 5.5)):
        for n1 in range(128, 256):                       # qb = n1 / 128 in [1, 2), kb = n2 / 128 in [0, 2)
            for n2 in range(1, 256):
                s = np.float32(qa * ka + (n1 / 128.0) * (n2 / 128.0))
                if float(s) != qa * ka + (n1 / 128.0) * (n2 / 128.0):
                    continue                             # (the fp32 accumulator must hold the score exactly)
                arg = np.float32(s * kexp)
                p = 2.0 ** float(arg)
                if float(arg) <= 16.0 and lo <= p <= 65536.0:
                    return (qa, n1 / 128.0), (ka, n2 / 128.0), float(s), float(arg), p
    return None


@pytest.mark.parametrize("T,wide,pipe", [(128, 0, 1), (512, 2, 0), (512, 2, 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_attention16_rescale_threshold_stays_finite_in_the_element_type(dtype, T, wide, pipe, tune):
    """The deferred rescale keeps the old reference while a tile's maximum outgrows it by at most 2^RESCALE_LOG2, and P is stored in the
    element type: at 2^16 an fp16 p in [65520, 65536] is +inf, the row sum inf and the output row NaN.  Identical queries (the
    wave-uniform `grow` stays false), zero keys in the first 64-key tile, ONE key of the second tile with a score inside that window.
    With the threshold a property of the element type (15 for fp16) the row is finite and equals fp64 -- almost exactly V of that
    key.  Before the fix: every output row of the fp16 instantiation non-finite (recorded in the commit message)."""
    from mgea import ops
    found = _rescale_window_inputs()
    assert found is not None, "no fp16-exact score inside the window: the search is broken"
    (qa, qb), (ka, kb), s, arg, p = found
    assert arg <= 16.0 and 65520.0 <= p <= 65536.0
    print(f"[rescale window] q=({qa}, {qb}) k=({ka}, {kb}) raw score {s!r} arg {arg!r} p {p:.2f}")
    B, H, dh, big = 1, 2, 64, 77                                   # key 77: in the second 64-key tile of the first stage
    q = np.zeros((B, T, H, dh)); k = np.zeros((B, T, H, dh))
    q[..., 0], q[..., 1] = qa, qb
    k[:, big, :, 0], k[:, big, :, 1] = ka, kb
    v = _v_rows(B, T, H, dh)
    assert _exact16(q) and _exact16(k) and _exact16(v)
    valid = np.ones((B, T), dtype=bool)
    want = _ref64(q, k, v, valid)
    assert float(np.abs(want - v[:, big][:, None]).max()) < 2 * (T - 1) / p * 2.0      # ~ V of that key: the others weigh (T - 1) / p
    tune("attn16_wide", wide)
    tune("attn16_pipe", pipe)
    qkv = torch.from_numpy(np.concatenate([x.reshape(B, T, -1) for x in (q, k, v)], -1)).to(dtype)
    got = ops.attention16(qkv.cuda(), H).double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).any(-1).sum())} of {B * T * H} output rows are not finite"
    err = float(np.abs(got - want).max())
    print(f"[rescale window] {_ID[dtype]} T={T}: max |out - fp64| = {err:.3e}")
    # |V| <= 2: the output rounding (half an ulp at 2: 3.9e-3 bf16, 4.9e-4 fp16) is all that is left -- inside the diffuse-case bounds.
    # Observed on MI355X: bf16 3.9e-3, fp16 4.9e-4 (T = 128: 1.5e-4)
    assert err < DIFFUSE_BOUND[dtype]


# ---- the paged (decode / extend) attention ----------------------------------------------------------------------------------
MAX_PAGES = 16                                          # table width: > 4, so that the split form is taken at T = 1
CTX_PAIRS = [(1, 1000), (64, 65), (65, 257), (257, 64), (1000, 1)]


def _page_setup(B, n_head, dh, pdtype, arith, seed):
    """-> (image filled with poison [K slots 8, V slots 1024], page table [B, MAX_PAGES], arith_batch)"""
    from mgea import ops
    if arith:
        n_pages = MAX_PAGES * B
        table = np.arange(MAX_PAGES)[None, :] * B + np.arange(B)[:, None]
    else:
        n_pages = MAX_PAGES * B + 8
        table = np.random.RandomState(seed).permutation(n_pages)[:B * MAX_PAGES].reshape(B, MAX_PAGES)
    image = torch.empty(ops.kv_page_elems(n_pages, n_head, dh), dtype=pdtype)
    img = image.view(n_pages, 2, -1)
    img[:, 0] = 8.0
    img[:, 1] = 1024.0
    return image, table, (B if arith else 0)


def _paged_case_iter(family, lens_total, Tq, H, dh, nbits=NBITS):
    """the launches of one family, one at a time: one Case per round of pointer targets (a launch has only B * H * Tq queries); K | V
    are the same in every round"""
    L = max(lens_total)
    valid = np.arange(L)[None, :] < np.asarray(lens_total)[:, None]
    if family != "pointer":
        yield Case(family, valid, H, dh, Tq=Tq, nbits=nbits)
        return
    per_row = [_targets(valid[b], extra=[127, 128, 255, 256, 511, 512, 767, 768, (n - 1) // 64 * 64, n - 2])
               for b, n in enumerate(lens_total)]
    per_launch = H * Tq
    rounds = max((len(t) + per_launch - 1) // per_launch for t in per_row)
    for r in range(rounds):
        tg = [[[t[(r * per_launch + h * Tq + i) % len(t)] for i in range(Tq)] for h in range(H)] for t in per_row]
        yield Case(family, valid, H, dh, Tq=Tq, q_targets=tg, nbits=nbits)


@functools.lru_cache(maxsize=None)
def _paged_cases(family, lens_total, Tq, H, dh, nbits=NBITS):
    """the launches of one family, kept (the small shapes are shared between tests)"""
    return list(_paged_case_iter(family, lens_total, Tq, H, dh, nbits))


def _run_paged(case, pdtype, arith, split, ctx_len, lens, seed):
    from mgea import ops
    B, Tq = case.q.shape[:2]
    image, table, ab = _page_setup(B, case.H, case.dh, pdtype, arith, seed)
    k, v = (torch.from_numpy(x).to(pdtype) for x in (case.k, case.v))
    ops.kv_pages_write(image, k, v, table, valid=case.valid)
    qkv = torch.zeros(B, Tq, 3 * case.H * case.dh)
    qkv[..., :case.H * case.dh] = torch.from_numpy(case.q.reshape(B, Tq, -1)).float()
    qkv[..., case.H * case.dh:] = float("nan")                      # the kernel reads K | V from the pages only
    info = []
    out = ops.attention_paged(qkv.cuda(), case.H, image.cuda(), torch.from_numpy(table).cuda(), torch.tensor(ctx_len).cuda(),
                              None if lens is None else torch.tensor(lens).cuda(), arith_batch=ab, split=split, info=info)
    # which kernel ran: the split-context form spreads the 16 table pages of a decode query over 4 workgroups; never for T > 1
    assert info == [4 if split and Tq == 1 else 1], f"workgroups per query: {info}"
    return out


@pytest.mark.parametrize("ctx", CTX_PAIRS, ids=lambda c: f"ctx{c[0]}_{c[1]}")
@pytest.mark.parametrize("arith", [1, 0], ids=["arith", "table"])
@pytest.mark.parametrize("split", [0, 1], ids=["one_wg", "split"])
@pytest.mark.parametrize("pdtype,dh", [(torch.float32, 32), (torch.float32, 64), (torch.float32, 96), (torch.float32, 128),
                                       (torch.float16, 32), (torch.float16, 64), (torch.float16, 128)],
                         ids=lambda x: _ID.get(x, str(x)))
def test_attention_paged_counts_every_cached_key_exactly_once(pdtype, dh, split, arith, ctx):
    """One decode query per (row, head) over a host-built page image whose every unused slot -- the tail of the last page, the pages
    no row owns -- holds poison.  ctx = the tokens each of the two rows sees (its own token included, as in a decode step).  With the
    split scratch the launcher spreads the pages over several workgroups (switch attn_split at its default); arith: physical page
    j * B + b computed in the kernel, table: a random permutation into a larger pool, loaded from the table."""
    from mgea import _lib
    assert _lib.tune_get("attn_split") == 64 and _lib.tune_get("attn_arith_pages") == 1
    for family in FAMILIES:
        for case in _paged_cases(family, ctx, 1, 2, dh):
            out = _run_paged(case, pdtype, arith, bool(split), [c - 1 for c in ctx], None, seed=dh + ctx[0])
            case.check(out, torch.float32, what=f"dh={dh} ctx={ctx} split={split} arith={arith}")


@pytest.mark.parametrize("pdtype,dh", [(torch.float32, 32), (torch.float32, 64), (torch.float32, 96), (torch.float32, 128),
                                       (torch.float16, 32), (torch.float16, 64), (torch.float16, 128)],
                         ids=lambda x: _ID.get(x, str(x)))
def test_attention_paged_ragged_extend(pdtype, dh):
    """T = 3 new tokens per row, lens = [3, 1]: row 0 sees 62 + 3 cached tokens (across a page boundary), row 1 sees 130 + 1; the two
    padded queries of row 1 give zero rows."""
    ctx_len, lens = [62, 130], [3, 1]
    total = tuple(c + n for c, n in zip(ctx_len, lens))
    rows = np.arange(3)[None, :] < np.asarray(lens)[:, None]
    for family in FAMILIES:
        for case in _paged_cases(family, total, 3, 2, dh):
            out = _run_paged(case, pdtype, 0, True, ctx_len, lens, seed=dh)
            case.check(out, torch.float32, rows=rows, what=f"extend dh={dh}")
            assert float(out[1, 1:].abs().max()) == 0.0


# ---- the [CLS] attention of the last DistilBERT layer (csrc/attn_cls.hip) ---------------------------------------------------
# One query per (sequence, head); a wave walks its keys in blocks of 16 iterations x G key groups: G = 8 / blk = 128 keys at head_dim 64,
# G = 16 / blk = 256 at head_dim 32.  Three instantiations: <float, 64>, <__bf16, 64>, <float, 32>; all write fp32, and the 16-bit-exact
# inputs make the bf16 K | V lossless, so every one is held to ULP[fp32].
CLS_B, CLS_H = 4, 4
CLS_BLK = {64: 128, 32: 256}
CLS_S = {64: [1, 7, 8, 9, 127, 128, 129, 257, 300], 32: [1, 15, 16, 17, 255, 256, 257, 513]}
CLS_KINDS = ["none", "prefix", "random"]
CLS_FORMS = [(torch.float32, 64), (torch.bfloat16, 64), (torch.float32, 32)]
CLS_PACKED = (1, 20, 128, 129, 257)
CLS_PACKED_32 = (1, 20, 256, 257)       # head_dim 32: the poison family has 8 dims per sequence, and the block is 256 keys


def _cls_valid(kind, S, dh):
    """[CLS_B, S] bool.  prefix: lens [S, 1, min(blk, S), S - 1] (at least 1).  random, S > blk: row 0 has the kernel's whole first
    block masked and its first valid key at blk (the `mn == -inf -> continue` path, then alpha = exp(-inf)), row 1 has key 0 -- the
    [CLS] key itself -- masked, row 2 has a single valid key (the last: every earlier block is skipped), row 3 is plain random; S <= blk
    has no second block: key 0 valid in every row, row 2 keeps its single key."""
    blk = CLS_BLK[dh]
    if kind == "none":
        return np.ones((CLS_B, S), dtype=bool)
    if kind == "prefix":
        lens = [S, 1, min(blk, S), max(1, S - 1)]
        return np.arange(S)[None, :] < np.asarray(lens)[:, None]
    assert kind == "random"
    m = np.random.RandomState(2000 + 8 * S + dh).rand(CLS_B, S) > 0.3
    if S > blk:
        m[0, :blk] = False
        m[0, blk] = True
        m[1, 0] = False
        m[1, 1] = True
        m[2, :] = False
        m[2, S - 1] = True
        m[3, 0] = True
    else:
        m[:, 0] = True
        m[2, 1:] = False
    return m


@functools.lru_cache(maxsize=None)
def _cls_cases(family, kind, S, dh):
    """the launches of one family: a launch has only B * H queries, so the pointer family takes as many rounds as the pointer targets
    of the longest row need (as _paged_cases does)"""
    valid = _cls_valid(kind, S, dh)
    if family != "pointer":
        return [Case(family, valid, CLS_H, dh, Tq=1)]
    per_row = [_targets(valid[b], extra=[7, 8, 15, 16, 127, 128, 255, 256, S - 2]) for b in range(CLS_B)]
    rounds = max((len(t) + CLS_H - 1) // CLS_H for t in per_row)
    return [Case(family, valid, CLS_H, dh, Tq=1, q_targets=[[[t[(r * CLS_H + h) % len(t)]] for h in range(CLS_H)] for t in per_row])
            for r in range(rounds)]


def cls_case_list():
    """every (family, kind, S, head_dim) of the [CLS] tests (tests/test_bert_kernels_host.py builds them all on the CPU)"""
    return [(f, kind, S, dh) for dh in (64, 32) for S in CLS_S[dh] for kind in CLS_KINDS for f in FAMILIES]


def _cls_run(case, kv_dtype, mask):
    """q [B, D] fp32 and a qkv buffer whose q columns are NaN: the kernel reads K | V only"""
    from mgea import ops
    B, S = case.valid.shape
    D = case.H * case.dh
    qkv = torch.from_numpy(np.concatenate([np.full((B, S, D), np.nan)] + [x.reshape(B, S, D) for x in (case.k, case.v)], -1)).to(kv_dtype)
    q = torch.from_numpy(case.q.reshape(B, D)).float()
    return ops.attention_cls(q.cuda(), qkv.cuda(), case.H, mask=mask).view(B, 1, D)


@pytest.mark.parametrize("kind", CLS_KINDS)
@pytest.mark.parametrize("kv_dtype,dh", CLS_FORMS, ids=lambda x: _ID.get(x, str(x)))
def test_attention_cls_counts_every_valid_key_exactly_once(kv_dtype, dh, kind):
    for S in CLS_S[dh]:
        for family in FAMILIES:
            for case in _cls_cases(family, kind, S, dh):
                mask = None if kind == "none" else torch.from_numpy(case.valid).to(torch.int32).cuda()
                case.check(_cls_run(case, kv_dtype, mask), torch.float32, what=f"attn_cls {_ID[kv_dtype]} dh={dh} S={S} {kind} mask")


@pytest.mark.parametrize("kv_dtype,dh,seqs", [(torch.float32, 64, CLS_PACKED), (torch.bfloat16, 64, CLS_PACKED), (torch.float32, 32, CLS_PACKED_32)],
                         ids=lambda x: _ID.get(x, str(x) if isinstance(x, int) else "seqs"))
def test_attention_cls_packed_rows_stay_inside_their_sequence(kv_dtype, dh, seqs):
    """cu_seqlens input: the query of sequence s is the query of one of its own tokens in _packed_case (pointer: the code of that
    token's target, round r takes token r of every sequence so that all targets of the longest are visited); poison: the keys of the
    other sequences are loud and V is 2^s."""
    from mgea import ops
    H, C = 2, 2 * dh
    cu = np.concatenate([[0], np.cumsum(seqs)])
    for family in FAMILIES:
        qkv, exp = _packed_case(family, seqs, H, dh)
        kv = qkv.clone()
        kv[:, :C] = float("nan")
        kv = kv.to(kv_dtype).cuda()
        for r in range(16 if family == "pointer" else 1):
            tok = np.asarray([cu[s] + r % n for s, n in enumerate(seqs)])
            got = ops.attention_cls(qkv[tok, :C].cuda(), kv, H, cu=torch.from_numpy(cu).to(torch.int32).cuda()).double().cpu().numpy()
            want = exp[0, tok].reshape(len(seqs), C)
            tol = ULP[torch.float32] * (np.abs(want) if family != "pointer" else 1.0)
            bad = ~(np.abs(got - want) <= tol)
            assert not bad.any(), f"{family} round {r}: {int(bad.sum())} wrong outputs, first in sequence {int(np.nonzero(bad)[0][0])}"


@pytest.mark.parametrize("kv_dtype,dh", CLS_FORMS, ids=lambda x: _ID.get(x, str(x)))
def test_attention_cls_sequence_without_a_valid_key_gives_zeros(kv_dtype, dh):
    """The kernel's contract (_ref64 cannot express it): a sequence whose every key is masked, or a packed sequence of no rows, gives an
    all-zero, finite output row; its neighbours are untouched by it."""
    from mgea import ops
    for S in (1, CLS_BLK[dh] + 1, 300):
        case = Case("poison", np.ones((CLS_B, S), dtype=bool), CLS_H, dh, Tq=1)
        mask = torch.ones(CLS_B, S, dtype=torch.int32)
        mask[1] = 0
        out = _cls_run(case, kv_dtype, mask.cuda()).cpu()
        assert torch.equal(out[1], torch.zeros_like(out[1])), f"S={S}: the row without a valid key is not zero"
        rows = np.ones((CLS_B, 1), dtype=bool)
        rows[1] = False
        case.check(out, torch.float32, rows=rows, what=f"S={S}, row 1 fully masked")
    seqs = (20, 0, 129)
    H, C = 2, 2 * dh
    qkv, exp = _packed_case("poison", (20, 129), H, dh)
    cu = torch.tensor([0, 20, 20, 149], dtype=torch.int32)
    q = torch.stack([qkv[0, :C], qkv[0, :C], qkv[20, :C]])
    got = ops.attention_cls(q.cuda(), qkv.to(kv_dtype).cuda(), H, cu=cu.cuda()).cpu()
    assert torch.equal(got[1], torch.zeros(C)), f"packed {seqs}: the empty sequence's row is not zero"
    assert float((got[0] - 1.0).abs().max()) <= ULP[torch.float32] and float((got[2] - 2.0).abs().max()) <= 2 * ULP[torch.float32]


def test_attention_cls_refusals():
    from mgea import ops
    q, qkv = torch.zeros(2, 128).cuda(), torch.zeros(2, 4, 384).cuda()
    out = ops.attention_cls(q, qkv, 2)                      # the shape itself is fine
    assert out.shape == (2, 128)
    with pytest.raises(RuntimeError, match="no key mask"):
        ops.attention_cls(q, qkv.view(8, 384), 2, mask=torch.ones(2, 4, dtype=torch.int32).cuda(), cu=torch.tensor([0, 4, 8]).cuda())
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.attention_cls(q, qkv.bfloat16(), 4)             # bf16 with head_dim 32
    with pytest.raises(RuntimeError, match="not built"):
        ops.attention_cls(q, qkv, 1)                        # head_dim 128
    with pytest.raises(RuntimeError):
        ops.attention_cls(q, qkv.half(), 2)                 # fp16 K | V


# Diffuse softmax: uniform +-1.5 inputs (what test_attention_dense uses), rounded to bf16 first for the bf16 form, ragged prefix mask,
# against fp64.  The bound is the project's bound for the fp32 dense attention on this distribution.
CLS_DIFFUSE_BOUND = 2e-5


@pytest.mark.parametrize("kv_dtype,dh,S", [(torch.float32, 64, 300), (torch.bfloat16, 64, 300), (torch.float32, 32, 600)],
                         ids=lambda x: _ID.get(x, str(x)))
def test_attention_cls_diffuse_softmax_against_fp64(kv_dtype, dh, S):
    """Observed on MI355X: 4.9e-8 (f32, head_dim 64), 4.8e-8 (bf16 K | V), 3.0e-8 (head_dim 32)"""
    from mgea import ops
    B, H = CLS_B, CLS_H
    D = H * dh
    g = torch.Generator().manual_seed(11 + dh)
    qkv = ((torch.rand(B, S, 3 * D, generator=g) * 2 - 1) * 1.5).to(kv_dtype)
    qrow = ((torch.rand(B, D, generator=g) * 2 - 1) * 1.5).float()
    valid = _cls_valid("prefix", S, dh)
    k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, S, H, dh).double().numpy() for i in (1, 2))
    want = _ref64(qrow.reshape(B, 1, H, dh).double().numpy(), k, v, valid).reshape(B, D)
    got = ops.attention_cls(qrow.cuda(), qkv.cuda(), H, mask=torch.from_numpy(valid).to(torch.int32).cuda()).double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"[attention_cls diffuse] {_ID[kv_dtype]} dh={dh} S={S}: max |out - fp64| = {err:.3e} (bound {CLS_DIFFUSE_BOUND:.1e})")
    assert err < CLS_DIFFUSE_BOUND


# ---- the exact-fp32 dense attention ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [65, 129, 1000])
def test_attention_f32_counts_every_valid_key_exactly_once(T):
    from mgea import ops
    lens = np.asarray([T, max(1, T - 66)])
    valid = np.arange(T)[None, :] < lens[:, None]
    for family in FAMILIES:
        case = Case(family, valid, 2, 64)
        out = ops.attention(case.qkv().cuda(), 2, lens=torch.from_numpy(lens).cuda())
        case.check(out, torch.float32, what=f"fp32 dense T={T}")
