"""The kernels that end a decode step (csrc/step_tail.hip, the fused tail of csrc/sampler.hip, end_row_step / advance_embed_row /
embed_qkv0_row of csrc/common.h) and the row kernels around the decoder's prefill (embed_stats_kernel, embed_ln_kernel,
add_lens_kernel, take_last_kernel), each launched alone through mgea_op_step_tail / mgea_op_dec_embed / the bookkeeping wrappers and
held to the written rule of tests/step_tail_util.py (whose premises tests/test_step_tail_host.py proves on the CPU).

Every output buffer starts as poison, with poison in front of it and behind it, and is compared WHOLE: what a kernel must not touch is
asserted too.  Integer state is compared with torch.equal; x is bit-equal to the one fp32 add; the only tolerance is the fp32
row-operation bound 2e-5, for LayerNorm and the row statistics.

Observed on an MI355X (maxima over every case of this file):
    LayerNorm from the kernels' (mean, M2) against LayerNorm from the fp64 mean and variance      2.7e-7   (bound 2e-5)
    xn of embed_ln_kernel against ln64                                                            6.2e-7   (bound 2e-5)
The three producers of the next step's x / stats (embed_stats_kernel, argmax_advance_embed_kernel, the fused sampler tail) are
bit-equal on the same (id, pos): asserted below."""
import numpy as np
import pytest
import torch

import step_tail_util as U
from decode_gemm_util import permuted_table
from mgea import _lib, ops
from mgea.decoder import RowSampling

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
I32, F32 = torch.int32, torch.float32


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int64).astype(np.int32)))


def bits(t):
    return t.contiguous().view(I32).reshape(-1)


class Buf:
    """A device buffer between two poison pads; .t is the caller's view, check() compares pads and body as int32 bits."""

    def __init__(self, init):
        words = bits(init)
        self.n = words.numel()    # int32 words of the body
        pad = torch.full((PAD,), U.POISON, dtype=I32)
        self.full = torch.cat([pad, words, pad]).to(DEV)
        self.t = self.full[PAD:PAD + self.n].view(init.dtype)

    @classmethod
    def poison(cls, n, dtype=F32):
        return cls(poison_ints(n) if dtype == I32 else ops.poison(n, dtype))

    def cpu(self, dtype=None):
        t = self.full.cpu()[PAD:PAD + self.n]
        return t if dtype is None else t.view(dtype)

    def pads_intact(self, what):
        f = self.full.cpu()
        assert bool((f[:PAD] == U.POISON).all()) and bool((f[PAD + self.n:] == U.POISON).all()), f"{what}: written outside the buffer"

    def check(self, want, what):
        self.pads_intact(what)
        got, exp = self.cpu(), bits(want)
        assert got.numel() == exp.numel(), what
        if not torch.equal(got, exp):
            at = torch.nonzero(got != exp).reshape(-1)
            raise AssertionError(f"{what}: {at.numel()} of {exp.numel()} words differ, first at {at[:6].tolist()}: "
                                 f"got {got[at[:6]].tolist()} want {exp[at[:6]].tolist()}")


def poison_ints(n):
    return torch.full((int(n),), U.POISON, dtype=I32)


# ---- the rows' state and records from a scenario --------------------------------------------------------------------------------
N_DONE_START = 5   # the launch ADDS to the counter


class State:
    def __init__(self, sc, n_steps=U.N_STEPS, ids_out=True):
        B = len(sc["tok"])
        self.B, self.n_steps = B, n_steps
        self.cur_ids, self.ctx_len = Buf(i32(sc["fed"])), Buf(i32(sc["len"]))
        self.done, self.row_step = Buf(i32(sc["done"])), Buf(i32(sc["step"]))
        self.n_done = Buf(torch.tensor([N_DONE_START], dtype=I32))
        self.ids_out = Buf(poison_ints(B * n_steps)) if ids_out else None

    def args(self):
        return dict(cur_ids=self.cur_ids.t, ctx_len=self.ctx_len.t, done=self.done.t, row_step=self.row_step.t, n_done=self.n_done.t,
                    ids_out=None if self.ids_out is None else self.ids_out.t, n_steps=self.n_steps)

    def check(self, ex, what):
        self.cur_ids.check(i32(ex["cur_ids"]), what + ": cur_ids")
        self.ctx_len.check(i32(ex["ctx_len"]), what + ": ctx_len")
        self.done.check(i32(ex["done"]), what + ": done (1 finished, 2 parked)")
        self.row_step.check(i32(ex["row_step"]), what + ": row_step")
        self.n_done.check(torch.tensor([N_DONE_START + ex["n_done"]], dtype=I32), what + ": n_done")
        if self.ids_out is not None:
            self.ids_out.check(i32(ex["ids_out"]), what + ": ids_out")


def records(sc, penalty=None, bias=None):
    """(rows, ctx_cap) of a scenario: greedy rows (top_k = 1: the exact argmax of the processed row)"""
    rows = [RowSampling(1.0, 1, None, penalty, int(sc["eos"][j]), int(sc["max_new"][j]), 0,
                        logit_bias=None if bias is None else bias[j]) for j in range(len(sc["tok"]))]
    return rows, [int(c) for c in sc["cap"]]


def planted_partials(tok, n_tiles=3):
    """pval / pidx [B, n_tiles] whose merged argmax is tok[b]: the maximum sits in tile b mod n_tiles, the other tiles hold other ids"""
    B = len(tok)
    pval = np.tile(np.arange(n_tiles, dtype=np.float32), (B, 1))
    pidx = (np.asarray(tok)[:, None] + 1 + np.arange(n_tiles)[None, :]).astype(np.int32)
    w = np.arange(B) % n_tiles
    pval[np.arange(B), w] = U.WIN
    pidx[np.arange(B), w] = np.asarray(tok)
    return torch.from_numpy(pval).to(DEV), torch.from_numpy(pidx).to(DEV), n_tiles


VOCAB, POS_ROWS = 50, 64


def tables(C, seed=0):
    g = torch.Generator().manual_seed(1234 + seed)
    return torch.randn(VOCAB, C, generator=g), torch.randn(POS_ROWS, C, generator=g)


def expected_rows(tok_emb, pos_emb, fed, next_len, absolute_pos):
    ids = [U.embed_id(int(f), VOCAB) for f in fed]
    pos = [U.embed_position(int(n), absolute_pos, POS_ROWS) for n in next_len]
    return tok_emb[ids] + pos_emb[pos], ids      # ONE IEEE fp32 add per element: it has one answer


def tiled_image(rows):
    B, C = rows.shape
    img = ops.poison(U.tiled_floats(B, C))
    img[torch.from_numpy(U.tiled_offsets(B, C).reshape(-1))] = rows.reshape(-1)
    return img


def check_stats(buf, rows, what):
    """stats [B][4] = (mean, M2 / 2, mean, M2 / 2), and LayerNorm from them against LayerNorm from the fp64 moments"""
    buf.pads_intact(what)
    s = buf.cpu(F32).view(-1, 4)
    assert torch.equal(bits(s[:, 0]), bits(s[:, 2])) and torch.equal(bits(s[:, 1]), bits(s[:, 3])), f"{what}: the two half-row partials differ"
    a = U.ln_from_stats(rows.numpy(), s[:, 0].numpy(), 2.0 * s[:, 1].double().numpy())
    d = float(np.abs(a - U.ln64(rows.numpy())).max())
    print(f"OBSERVED {what}: LayerNorm from (mean, M2) vs fp64 {d:.3e}")
    assert d <= U.TOL, f"{what}: LayerNorm from the kernel's statistics is {d:.3g} off the fp64 one (bound {U.TOL})"


class Embed:
    """the next step's embedding buffers of a fused tail: x (k-tiled) + stats, or the qkv0 table form"""

    def __init__(self, B, C, absolute_pos=1, table=None, seed=0):
        self.B, self.C, self.absolute_pos = B, C, absolute_pos
        self.tok_emb, self.pos_emb = tables(C, seed)
        self.x, self.stats = Buf.poison(U.tiled_floats(B, C)), Buf.poison(4 * B)
        self.d_tok, self.d_pos = self.tok_emb.to(DEV), self.pos_emb.to(DEV)
        self.table = table
        if table is not None:
            H, dh, mp = table["n_head"], table["head_dim"], table["max_pages"]
            assert H * dh == C
            self.arith = table.get("arith_batch", 0)
            self.n_pages = table.get("n_pages", mp * max(B, self.arith))
            self.pt = (np.arange(mp)[None, :] * self.arith + np.arange(B)[:, None]).astype(np.int32) if self.arith else \
                permuted_table(B, mp, self.n_pages)
            g = torch.Generator().manual_seed(99 + seed)
            self.qkv0 = torch.randn(VOCAB, 3 * C, generator=g)
            self.d_qkv0, self.d_pt = self.qkv0.to(DEV), torch.from_numpy(self.pt).to(DEV)
            self.qkv = Buf.poison(B * 3 * C)
            self.pages = Buf.poison(ops.kv_page_elems(self.n_pages, H, dh), table.get("dtype", F32))

    def args(self):
        e = dict(tok_emb=self.d_tok, pos_emb=self.d_pos, x=self.x.t, stats=self.stats.t, C=self.C, vocab=VOCAB, pos_rows=POS_ROWS,
                 absolute_pos=self.absolute_pos)
        if self.table is None:
            return dict(embed=e)
        t = dict(qkv0=self.d_qkv0, qkv=self.qkv.t, pages=self.pages.t, n_pages=self.n_pages, n_head=self.table["n_head"],
                 head_dim=self.table["head_dim"], page_table=self.d_pt, arith_batch=self.arith)
        return dict(embed=e, table=t)

    def check(self, fed, next_len, what):
        rows, ids = expected_rows(self.tok_emb, self.pos_emb, fed, next_len, self.absolute_pos)
        self.x.check(tiled_image(rows), what + ": x (bit-equal to the fp32 sum)")
        if self.table is None:
            check_stats(self.stats, rows, what + ": stats")
            return rows
        self.stats.check(ops.poison(4 * self.B), what + ": stats must stay untouched in the table form")
        self.qkv.check(self.qkv0[ids], what + ": qkv = the table row")
        H, dh = self.table["n_head"], self.table["head_dim"]
        img = ops.poison(ops.kv_page_elems(self.n_pages, H, dh))
        kv = self.qkv0[ids][:, self.C:]
        ops.kv_pages_write(img, kv[:, :self.C].reshape(self.B, 1, H, dh), kv[:, self.C:].reshape(self.B, 1, H, dh), self.pt,
                           pos0=[int(n) for n in next_len])
        self.pages.check(img, what + ": layer-0 page image")
        return rows


# ---- end of step: every caller against the one rule -------------------------------------------------------------------------------
BATCHES = (1, 64, 255, 256, 257, 512)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("form", ["records", "by_value", "by_value_no_eos"])
def test_advance_kernels_follow_the_rule(B, form):
    """advance_kernel<false / true> and advance_scored_kernel<false / true>, one thread per row, ceil(B / 256) blocks"""
    rec = form == "records"
    eos = {"records": -1, "by_value": U.EOS, "by_value_no_eos": -1}[form]
    sc = U.scenarios(B, rec)
    ex = U.expected_state(sc, rec, eos_by_value=eos)
    rows, caps = records(sc) if rec else (None, None)
    V = 40 + 3          # every scenario token is an id of it; 43 is no multiple of 32
    start_bits = ops.pack_presence([[(3 * j) % V, 1] for j in range(B)], B, V).view(np.int32)
    want_bits = start_bits.copy().view(np.uint32)
    for j in range(B):
        if U.presence_bit_set(int(sc["tok"][j]), int(sc["done"][j]), V):
            want_bits[j, int(sc["tok"][j]) >> 5] |= np.uint32(1) << np.uint32(int(sc["tok"][j]) & 31)
    stride = U.N_STEPS - 1   # shorter than ids_out: step == stride is written to ids_out and filed nowhere
    lp_step = torch.arange(B, dtype=F32) * 0.25 - 3.5
    ch_step = -(torch.arange(B, dtype=F32) * 0.5) - 1.0
    want_lp, want_ch = ops.poison(B * stride).view(B, stride).clone(), ops.poison(B * stride).view(B, stride).clone()
    for j in range(B):
        for want, val in ((want_lp, lp_step), (want_ch, ch_step)):
            e = U.score_entry(int(sc["step"][j]), int(sc["done"][j]), float(val[j]), stride)
            if e is not None:
                want[j, e[0]] = e[1]
    for penalty in (False, True):
        for scored in (False, True):
            what = f"advance{'_scored' if scored else ''}_kernel<{str(penalty).lower()}> B={B} {form}"
            st, sampled = State(sc), Buf(i32(sc["tok"]))
            pres = Buf(torch.from_numpy(start_bits.copy()).reshape(-1)) if penalty else None
            lph, chh = Buf.poison(B * stride), Buf.poison(B * stride)
            scores = dict(logprob_step=lp_step.to(DEV), choice_step=ch_step.to(DEV), logprob_hist=lph.t, choice_hist=chh.t, stride=stride) if scored else None
            ops.step_tail(_lib.TAIL_ADVANCE, B, st.args(), rows=rows, ctx_cap=caps, eos_id=eos, sampled=sampled.t,
                          presence=None if pres is None else pres.t, V=V, scores=scores)
            st.check(ex, what)
            sampled.check(i32(sc["tok"]), what + ": sampled is read only")
            if penalty:
                pres.check(torch.from_numpy(want_bits.view(np.int32)).reshape(-1), what + ": presence")
            lph.check(want_lp if scored else ops.poison(B * stride), what + ": logprob history")
            chh.check(want_ch if scored else ops.poison(B * stride), what + ": choice history")


@pytest.mark.parametrize("B", [1, 257, 512])
@pytest.mark.parametrize("form", ["records", "by_value", "by_value_no_eos"])
def test_argmax_tails_follow_the_rule(B, form):
    """argmax_advance_kernel and both forms of argmax_advance_embed_kernel leave the state advance_kernel leaves"""
    rec = form == "records"
    eos = {"records": -1, "by_value": U.EOS, "by_value_no_eos": -1}[form]
    sc = U.scenarios(B, rec)
    ex = U.expected_state(sc, rec, eos_by_value=eos)
    rows, caps = records(sc) if rec else (None, None)
    part = planted_partials(sc["tok"])
    st, sampled = State(sc), Buf.poison(B, I32)
    ops.step_tail(_lib.TAIL_ARGMAX, B, st.args(), rows=rows, ctx_cap=caps, eos_id=eos, partials=part, sampled=sampled.t)
    st.check(ex, f"argmax_advance_kernel B={B} {form}")
    sampled.check(i32(sc["tok"]), "argmax_advance_kernel: sampled")
    for table in (None, dict(n_head=2, head_dim=32, max_pages=2, arith_batch=B)):
        what = f"argmax_advance_embed_kernel ({'table' if table else 'stats'} form) B={B} {form}"
        st, sampled = State(sc), Buf.poison(B, I32)
        em = Embed(B, 64 if table else 128, absolute_pos=1, table=table)
        ops.step_tail(_lib.TAIL_ARGMAX_EMBED, B, st.args(), rows=rows, ctx_cap=caps, eos_id=eos, partials=part, sampled=sampled.t, **em.args())
        st.check(ex, what)
        sampled.check(i32(sc["tok"]), what + ": sampled")
        em.check(ex["fed"], ex["next_len"], what)


# ---- the fused sampler tail ---------------------------------------------------------------------------------------------------------
def small_logits(B, V):
    return ((torch.arange(V)[None, :] * 7 + torch.arange(B)[:, None] * 3) % 23).float()   # integers below 23: WIN towers above them


def other_id(tok, V, k):
    return (int(tok) + k) % V


@pytest.mark.parametrize("B", [1, 512])
@pytest.mark.parametrize("form", ["plain", "plain_table", "penalty", "bias", "scored", "scored_no_choice", "grammar", "scored_grammar"])
def test_fused_sampler_tail_follows_the_rule(B, form):
    """sample_kernel with fuse_tail = 1 in its plain, PENALTY, BIAS, scored and GRAMMAR instantiations: greedy records (top_k = 1) take
    the exact argmax of a planted maximum, scored rows also take forced ids; the state it leaves is the rule's, as for every other caller"""
    V = VOCAB
    sc = U.scenarios(B, True)
    ex = U.expected_state(sc, True)
    tok, running = sc["tok"], ex["running"]
    lg = small_logits(B, V)
    at = np.asarray(tok).copy()                     # where the raw maximum is planted
    bias, penalty, start_bits, forced = None, None, None, None
    if form == "penalty":                           # a seen decoy above the token: only the penalty (/ 1.5) puts the token first
        penalty = 1.5
        decoy = [other_id(t, V, 11) for t in tok]
        lg[torch.arange(B), torch.tensor(decoy)] = U.WIN * 1.25
        start_bits = ops.pack_presence([[d] for d in decoy], B, V).view(np.int32)
    if form == "bias":                              # even rows: the raw maximum is elsewhere, their bias puts the token first
        bias = [({int(t): 2 * U.WIN} if j % 2 == 0 else None) for j, t in enumerate(tok)]
        at = np.asarray([other_id(t, V, 1) if j % 2 == 0 else t for j, t in enumerate(tok)])
    if form.startswith("scored"):                   # every third row is told its id, the raw maximum is elsewhere
        forced = np.asarray([int(t) if j % 3 == 0 else -1 for j, t in enumerate(tok)])
        at = np.asarray([other_id(t, V, 7) if j % 3 == 0 else t for j, t in enumerate(tok)])
    lg[torch.arange(B), torch.from_numpy(at)] = U.WIN
    n_state, n_class = 7, 5
    gram = None
    if "grammar" in form:
        class_of = np.arange(V) % n_class
        s_, c_ = np.arange(n_state)[:, None], np.arange(n_class)[None, :]
        nxt = np.where((s_ + c_) % 4 == 3, -1, (2 * s_ + c_ + 1) % n_state).astype(np.int32)
        states = np.zeros(B, np.int64)
        for j in range(B):
            if j % 5 == 4:
                states[j] = -1                      # a row without a grammar
                continue
            s = next(s for s in ((j + k) % n_state for k in range(n_state)) if nxt[s, class_of[tok[j]]] >= 0)
            states[j] = s
            if running[j] and forced is None:       # a banned id above the token: only the mask puts the token first
                banned = int(np.flatnonzero(nxt[s] < 0)[0])
                lg[j, banned] = U.WIN + 1
        want_states = states.copy()
        for j in range(B):
            if running[j] and states[j] >= 0:
                want_states[j] = nxt[states[j], class_of[tok[j]]]
        st_buf = Buf(i32(states))
        gram = dict(class_of=i32(class_of).to(DEV), next=torch.from_numpy(nxt).to(DEV).reshape(-1), n_state=n_state, n_class=n_class, states=st_buf.t)
    rows, caps = records(sc, penalty=penalty, bias=bias)
    table = dict(n_head=2, head_dim=32, max_pages=2, arith_batch=B) if form == "plain_table" else None
    st, sampled = State(sc), Buf.poison(B, I32)
    em = Embed(B, 64 if table else 128, absolute_pos=1, table=table)
    pres = Buf(torch.from_numpy(start_bits.copy()).reshape(-1)) if start_bits is not None else None
    stride = U.N_STEPS - 1
    lph, chh, err = Buf.poison(B * stride), Buf.poison(B * stride), Buf(torch.zeros(1, dtype=I32))
    scores = None
    if forced is not None:
        scores = dict(logprob_hist=lph.t, choice_hist=None if form == "scored_no_choice" else chh.t, stride=stride, forced=i32(forced).to(DEV))
    d_lg = lg.to(DEV)
    what = f"fused sampler tail ({form}) B={B}"
    ops.step_tail(_lib.TAIL_SAMPLE, B, st.args(), rows=rows, ctx_cap=caps, sampled=sampled.t, presence=None if pres is None else pres.t,
                  scores=scores, sampler=dict(logits=d_lg), grammar=gram, err_flag=err.t, **em.args())
    st.check(ex, what)
    sampled.check(i32(tok), what + ": sampled")
    em.check(ex["fed"], ex["next_len"], what)
    err.check(torch.zeros(1, dtype=I32), what + ": error flags")
    if pres is not None:
        want = start_bits.copy().view(np.uint32)
        for j in range(B):
            if U.presence_bit_set(int(tok[j]), int(sc["done"][j]), V):
                want[j, int(tok[j]) >> 5] |= np.uint32(1) << np.uint32(int(tok[j]) & 31)
        pres.check(torch.from_numpy(want.view(np.int32)).reshape(-1), what + ": presence")
    if gram is not None:
        st_buf.check(i32(want_states), what + ": grammar states (a finished row and a row at -1 keep theirs)")
    if forced is None:
        lph.check(ops.poison(B * stride), what + ": no history without the scored form")
        return
    # the values: log-softmax of the RAW row at the id is x_id - WIN exactly (every other exp underflows to 0); the choice value is
    # log 1 = 0 for the kept id and -inf for a forced id outside the kept set
    want_lp, want_ch = ops.poison(B * stride).view(B, stride).clone(), ops.poison(B * stride).view(B, stride).clone()
    for j in range(B):
        lp = float(lg[j, int(tok[j])]) - U.WIN
        for want, val in ((want_lp, lp), (want_ch, 0.0 if int(at[j]) == int(tok[j]) else -np.inf)):
            e = U.score_entry(int(sc["step"][j]), int(sc["done"][j]), val, stride)
            if e is not None:
                want[j, e[0]] = e[1]

    def same_values(buf, want, name):
        buf.pads_intact(name)
        got = buf.cpu(F32).view(B, stride)
        filed = bits(want).view(B, stride) != U.POISON
        assert torch.equal(bits(got).view(B, stride)[~filed], bits(want).view(B, stride)[~filed]), f"{name}: written where nothing is filed"
        assert torch.equal(got[filed], want[filed]), f"{name}: filed values"
    same_values(lph, want_lp, what + ": logprob history")
    if form == "scored_no_choice":
        chh.check(ops.poison(B * stride), what + ": choice is NULL")
        return
    if gram is not None:      # (the mask may leave the token as the kept id: the choice value is not planted here)
        chh.pads_intact(what + ": choice history")
        return
    same_values(chh, want_ch, what + ": choice history")
    # the unfused pair: the sampler's [B] vectors, then advance_scored_kernel -- the same histories bit for bit
    ids_u, lp_u, ch_u = ops.sample_rows_scored(d_lg, rows, step=0, forced=i32(forced))
    assert torch.equal(ids_u.cpu(), i32(tok))
    st2, lph2, chh2 = State(sc), Buf.poison(B * stride), Buf.poison(B * stride)
    ops.step_tail(_lib.TAIL_ADVANCE, B, st2.args(), rows=rows, ctx_cap=caps, sampled=ids_u,
                  scores=dict(logprob_step=lp_u, choice_step=ch_u, logprob_hist=lph2.t, choice_hist=chh2.t, stride=stride))
    st2.check(ex, what + ": the unfused pair")
    lph2.check(lph.cpu(F32), what + ": unfused logprob history is not the fused one bit for bit")
    chh2.check(chh.cpu(F32), what + ": unfused choice history is not the fused one bit for bit")


def test_forced_id_beyond_the_vocabulary_is_clamped_and_flagged():
    B, V = 4, VOCAB
    sc = dict(tok=np.asarray([V - 1, V - 1, 9, 3]), step=np.asarray([0, 1, 2, 3]), fed=np.full(4, 1), len=np.full(4, 5), done=np.zeros(4, np.int64),
              eos=np.full(4, -1), max_new=np.zeros(4, np.int64), cap=np.full(4, U.NONE))
    ex = U.expected_state(sc, True)
    lg = small_logits(B, V)
    lg[:, 9] = U.WIN
    forced = i32([V, V + 100, -1, 3])
    for with_flag in (True, False):
        st, sampled, em = State(sc), Buf.poison(B, I32), Embed(B, 32)
        lph, err = Buf.poison(B * 4), Buf(torch.zeros(1, dtype=I32))
        ops.step_tail(_lib.TAIL_SAMPLE, B, st.args(), rows=records(sc)[0], sampled=sampled.t, sampler=dict(logits=lg.to(DEV)),
                      scores=dict(logprob_hist=lph.t, choice_hist=None, stride=4, forced=forced.to(DEV)), err_flag=err.t if with_flag else None,
                      **em.args())
        st.check(ex, "forced >= V")
        sampled.check(i32(sc["tok"]), "forced >= V: the id becomes V - 1")
        err.check(torch.tensor([1 if with_flag else 0], dtype=I32), "forced >= V: bit 0 of the error flag")


# ---- partial argmax -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", U.TILE_COUNTS)
def test_partial_argmax(nt):
    """argmax_advance_kernel (64 lanes) and argmax_advance_embed_kernel (4 waves + LDS merge): one row per winner tile, exact ties
    across lanes and waves with the lower id in the later tile, rows of -inf, NaN partials"""
    pval, pidx, names = U.argmax_inputs(nt)
    want, ok = U.argmax_rule(pval, pidx)
    assert ok
    B = len(want)
    sc = dict(tok=want, step=np.zeros(B, np.int64), fed=np.full(B, 1), len=np.full(B, 1), done=np.zeros(B, np.int64))
    ex = U.expected_state(sc, False, eos_by_value=-1, n_steps=1)
    part = (torch.from_numpy(pval).to(DEV).reshape(-1), torch.from_numpy(pidx).to(DEV).reshape(-1), nt)
    for kind in (_lib.TAIL_ARGMAX, _lib.TAIL_ARGMAX_EMBED):
        st, sampled = State(sc, n_steps=1), Buf.poison(B, I32)
        em = Embed(B, 32, absolute_pos=0) if kind == _lib.TAIL_ARGMAX_EMBED else None
        ops.step_tail(kind, B, st.args(), eos_id=-1, partials=part, sampled=sampled.t, **(em.args() if em else {}))
        got = sampled.cpu().tolist()
        bad = [(names[r], got[r], int(want[r])) for r in range(B) if got[r] != want[r]]
        assert not bad, f"kind {kind}, {nt} tiles: (row, got, want) {bad}"
        sampled.pads_intact("sampled")
        st.check(ex, f"kind {kind}, {nt} tiles")
        if em:
            em.check(ex["fed"], ex["next_len"], f"argmax + embed, {nt} tiles (ids beyond the vocabulary are clamped)")


# ---- presence ---------------------------------------------------------------------------------------------------------------------
VOCABS = (31, 32, 33, 8324, 14336)


@pytest.mark.parametrize("V", VOCABS)
def test_presence_bit_of_the_step(V):
    """advance_kernel<true>: the bit of tok for a running row, none for a finished or parked row, nothing for tok outside [0, V),
    a word that has bits keeps them"""
    toks = [t for t in (0, 30, 31, 32, V - 1, V, V + 40, -1, 5) if t < V + 41]
    rows = [(t, d) for t in toks for d in (0, 1, 2)]
    B = len(rows)
    sc = dict(tok=np.asarray([t for t, _ in rows]), step=np.zeros(B, np.int64), fed=np.full(B, 1), len=np.full(B, 3),
              done=np.asarray([d for _, d in rows]))
    ex = U.expected_state(sc, False, eos_by_value=-1, n_steps=2)
    start = ops.pack_presence([[5 % V, (V - 1) // 2] for _ in range(B)], B, V).view(np.int32)
    want = start.copy().view(np.uint32)
    for j, (t, d) in enumerate(rows):
        if U.presence_bit_set(t, d, V):
            want[j, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    st, pres = State(sc, n_steps=2), Buf(torch.from_numpy(start.copy()).reshape(-1))
    ops.step_tail(_lib.TAIL_ADVANCE, B, st.args(), eos_id=-1, sampled=i32(sc["tok"]).to(DEV), presence=pres.t, V=V)
    st.check(ex, f"advance_kernel<true> V={V}")
    pres.check(torch.from_numpy(want.view(np.int32)).reshape(-1), f"presence V={V}")


@pytest.mark.parametrize("V", VOCABS)
def test_presence_bit_of_the_fused_tail(V):
    """sample_kernel<36 / 56, PENALTY> with its tail (8324: the 36-wide instantiation, ragged last word; 14336: the 56-wide one):
    tokens 0, 31, 32, V - 1 as far as the vocabulary has them"""
    toks = sorted({t for t in (0, 30, 31, 32, V - 1) if t < V})
    rows = [(t, d) for t in toks for d in (0, 1, 2)]
    B = len(rows)
    sc = dict(tok=np.asarray([t for t, _ in rows]), step=np.zeros(B, np.int64), fed=np.full(B, 1), len=np.full(B, 3),
              done=np.asarray([d for _, d in rows]), eos=np.full(B, -1), max_new=np.zeros(B, np.int64), cap=np.full(B, U.NONE))
    ex = U.expected_state(sc, True, n_steps=2)
    lg = small_logits(B, V)
    lg[torch.arange(B), torch.from_numpy(sc["tok"])] = U.WIN
    start = ops.pack_presence([[1, (V - 1) // 2] for _ in range(B)], B, V).view(np.int32)
    want = start.copy().view(np.uint32)
    for j, (t, d) in enumerate(rows):
        if U.presence_bit_set(t, d, V):
            want[j, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    g = torch.Generator().manual_seed(3)
    tok_emb, pos_emb = torch.randn(V, 32, generator=g), torch.randn(POS_ROWS, 32, generator=g)
    x, stats = Buf.poison(U.tiled_floats(B, 32)), Buf.poison(4 * B)
    st, sampled, pres = State(sc, n_steps=2), Buf.poison(B, I32), Buf(torch.from_numpy(start.copy()).reshape(-1))
    ops.step_tail(_lib.TAIL_SAMPLE, B, st.args(), rows=records(sc, penalty=1.25)[0], sampled=sampled.t, presence=pres.t,
                  sampler=dict(logits=lg.to(DEV)),
                  embed=dict(tok_emb=tok_emb.to(DEV), pos_emb=pos_emb.to(DEV), x=x.t, stats=stats.t, C=32, vocab=V, pos_rows=POS_ROWS, absolute_pos=0))
    st.check(ex, f"fused PENALTY tail V={V}")
    sampled.check(i32(sc["tok"]), "sampled")
    pres.check(torch.from_numpy(want.view(np.int32)).reshape(-1), f"presence V={V}")
    x.check(tiled_image(tok_emb[ex["fed"]] + pos_emb[0]), "x")


@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("V", VOCABS)
def test_presence_seed(V, T):
    """presence_seed_kernel against ops.pack_presence: repeated ids, ids outside [0, V) skipped, lens NULL / 0 / negative / above T,
    and a bitmap left by an earlier generation is cleared"""
    rs = np.random.RandomState(V + T)
    B = 7
    ids = rs.randint(0, V, size=(B, T))
    ids[:, ::3] = ids[:, :1]                               # repeats
    ids[1, ::5], ids[2, ::4], ids[3, ::2] = -1, V, V + 5   # outside the vocabulary
    lens_list = [T, 0, -3, T + 9, max(T // 2, 1), 1, T]
    W = ops.presence_words(V)
    for lens in (None, lens_list):
        n = [T] * B if lens is None else [min(max(l, 0), T) for l in lens]
        want = ops.pack_presence([[int(i) for i in ids[b, :n[b]] if 0 <= i < V] for b in range(B)], B, V)
        pres = Buf(torch.full((B * W,), -1, dtype=I32))    # every bit set by an "earlier generation"
        ops.presence_seed(i32(ids).to(DEV), None if lens is None else i32(lens).to(DEV), V, pres.t)
        pres.check(torch.from_numpy(want.view(np.int32)).reshape(-1), f"presence_seed V={V} T={T} lens={'NULL' if lens is None else 'given'}")
    pres = Buf.poison(B * W, I32)
    with pytest.raises(RuntimeError):
        ops.presence_seed(i32(ids).to(DEV), None, 14337, pres.t)
    pres.check(poison_ints(B * W), "a refused vocabulary launches nothing")


# ---- grammar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class", [1, 31, 32, 33, 4096])
def test_grammar_allow(n_class):
    """grammar_allow_kernel against next >= 0 packed on the host, n_state up to the cell cap"""
    for n_state in sorted({1, 3, min(4096, (1 << 20) // n_class)}):
        rs = np.random.RandomState(n_class + n_state)
        nxt = rs.randint(-1, n_state, size=(n_state, n_class)).astype(np.int32)
        nxt[:, -1] = np.where(np.arange(n_state) % 2 == 0, 0, -1)      # the last class (bit 31 of a full word) both ways
        W = (n_class + 31) // 32
        ok = np.concatenate([nxt >= 0, np.zeros((n_state, W * 32 - n_class), bool)], 1).reshape(n_state, W, 32)
        want = (ok.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
        allow = Buf.poison(n_state * W, I32)
        ops.grammar_allow(torch.from_numpy(nxt).to(DEV), allow.t)
        allow.check(torch.from_numpy(want.view(np.int32)).reshape(-1), f"allow {n_state} x {n_class}")


@pytest.mark.parametrize("shape", [(4097, 1), (1, 4097), (512, 4096)])
def test_grammar_allow_refusals(shape):
    allow = Buf.poison(4096, I32)
    with pytest.raises(RuntimeError):
        ops.grammar_allow(torch.zeros(shape, dtype=I32, device=DEV), allow.t)
    allow.check(poison_ints(4096), "a refused grammar launches nothing")


# ---- the next step's embedding --------------------------------------------------------------------------------------------------
WIDTHS = (4, 128, 1024, 1028, 4096)    # 1, 32, 256, 257 and 1024 float4 per row


def finished_rows(ids, pos):
    """rows that were finished before the step: a fused tail then embeds (cur_ids, ctx_len) as they are"""
    B = len(ids)
    return dict(tok=np.full(B, 7), step=np.zeros(B, np.int64), fed=np.asarray(ids), len=np.asarray(pos), done=np.ones(B, np.int64),
                eos=np.full(B, -1), max_new=np.zeros(B, np.int64), cap=np.full(B, U.NONE))


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("absolute_pos", [0, 1])
def test_three_producers_of_x_and_stats_are_bit_equal(C, absolute_pos):
    """embed_stats_kernel, argmax_advance_embed_kernel and the fused sampler tail on the same (id, pos): x bit-equal to the fp32 sum
    (ids clamped to the vocabulary, pos to pos_rows - 1), stats within 2e-5 of fp64 and the three results bit-equal to each other"""
    ids = [0, 49, 7, -2, 53, 21, 7]
    pos = [0, 1, 63, 64, 200, 17, 5]
    B = len(ids)
    tok_emb, pos_emb = tables(C, seed=C)
    rows, _ = expected_rows(tok_emb, pos_emb, ids, pos, absolute_pos)
    results = {}
    # embed_stats_kernel: T = 1, pos = ctx_len when absolute
    x, stats, err = Buf.poison(U.tiled_floats(B, C)), Buf.poison(4 * B), Buf(torch.zeros(1, dtype=I32))
    ops.dec_embed(0, i32(ids).view(B, 1).to(DEV), tok_emb.to(DEV), pos_emb.to(DEV), x.t, stats.t, ctx_len=i32(pos).to(DEV), absolute_pos=absolute_pos,
                  err_flag=err.t)
    err.check(torch.ones(1, dtype=I32), "embed_stats_kernel: bit 0 for the clamped ids")
    results["embed_stats_kernel"] = (x, stats)
    sc = finished_rows(ids, pos)
    for name, kind in (("argmax_advance_embed_kernel", _lib.TAIL_ARGMAX_EMBED), ("fused sampler tail", _lib.TAIL_SAMPLE)):
        st, sampled = State(sc), Buf.poison(B, I32)
        em = Embed(B, C, absolute_pos=absolute_pos, seed=C)
        lg = small_logits(B, VOCAB)
        lg[:, 7] = U.WIN
        extra = dict(partials=planted_partials(sc["tok"])) if kind == _lib.TAIL_ARGMAX_EMBED else dict(sampler=dict(logits=lg.to(DEV)))
        ops.step_tail(kind, B, st.args(), rows=records(sc)[0], sampled=sampled.t, **extra, **em.args())
        st.check(U.expected_state(sc, True), name)
        results[name] = (em.x, em.stats)
    for name, (x, stats) in results.items():
        x.check(tiled_image(rows), f"{name} C={C}: x")
        check_stats(stats, rows, f"{name} C={C}")
        assert torch.equal(stats.cpu(), results["embed_stats_kernel"][1].cpu()), f"{name}: stats differ in bits from embed_stats_kernel's"
    if C % 32 == 0:
        assert torch.equal(bits(ops.untile_rows(results["embed_stats_kernel"][0].t, B, C).cpu()), bits(rows))


@pytest.mark.parametrize("C", WIDTHS)
def test_prefill_embedding_kernels(C):
    """embed_stats_kernel and embed_ln_kernel on [B, T] prompts: T = 1 and ragged T > 1, rows past lens[b] are zero rows (xn = ln_b,
    stats = 0), absolute_pos 0 / 1 with ctx_len NULL / given, clamped ids flag real rows only"""
    tok_emb, pos_emb = tables(C, seed=C + 1)
    g = torch.Generator().manual_seed(C)
    ln_w, ln_b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    cases = [dict(B=5, T=1, lens=None, ctx=None, ap=0, bad=None),
             dict(B=3, T=4, lens=[4, 2, 0], ctx=[0, 61, 3], ap=1, bad=(0, 1)),      # a bad id in a real row
             dict(B=3, T=4, lens=[3, 1, 4], ctx=None, ap=1, bad=(1, 2)),            # a bad id past the row's length: no flag
             dict(B=2, T=5, lens=[5, 3], ctx=[70, 2], ap=0, bad=None)]
    for c in cases:
        B, T = c["B"], c["T"]
        M = B * T
        ids = (np.arange(M).reshape(B, T) * 7 + 3) % VOCAB
        if c["bad"]:
            ids[c["bad"]] = VOCAB + 4
            ids[0, 0] = -1 if c["bad"] == (0, 1) else ids[0, 0]
        lens = c["lens"] or [T] * B
        want = torch.zeros(M, C)
        flag = 0
        for b in range(B):
            for t in range(T):
                if t < lens[b]:
                    p = min(t + (c["ctx"][b] if (c["ap"] and c["ctx"]) else 0), POS_ROWS - 1)
                    flag |= int(not 0 <= ids[b, t] < VOCAB)
                    want[b * T + t] = tok_emb[U.embed_id(int(ids[b, t]), VOCAB)] + pos_emb[p]
        real = torch.tensor([t < lens[b] for b in range(B) for t in range(T)])
        kw = dict(lens=None if c["lens"] is None else i32(lens).to(DEV), ctx_len=None if c["ctx"] is None else i32(c["ctx"]).to(DEV), absolute_pos=c["ap"])
        d_ids, what = i32(ids).to(DEV), f"C={C} {c}"
        # embed_stats_kernel
        x, stats, err = Buf.poison(U.tiled_floats(M, C)), Buf.poison(4 * M), Buf(torch.zeros(1, dtype=I32))
        ops.dec_embed(0, d_ids, tok_emb.to(DEV), pos_emb.to(DEV), x.t, stats.t, err_flag=err.t, **kw)
        x.check(tiled_image(want), "embed_stats_kernel x " + what)
        err.check(torch.tensor([flag], dtype=I32), "embed_stats_kernel err_flag " + what)
        s = stats.cpu(F32).view(M, 4)
        assert bool((s[~real] == 0).all()), "stats of a zero row are 0"
        if real.any():
            keep = torch.nonzero(real).reshape(-1)
            sub = Buf(s[keep].reshape(-1).clone())
            check_stats(sub, want[keep], "embed_stats_kernel stats " + what)
        stats.pads_intact("stats")
        # embed_ln_kernel, with and without the LayerNorm
        for with_ln in (True, False):
            x, xn, err = Buf.poison(M * C), Buf.poison(M * C), Buf(torch.zeros(1, dtype=I32))
            ops.dec_embed(1, d_ids, tok_emb.to(DEV), pos_emb.to(DEV), x.t, xn.t, ln_w=ln_w.to(DEV) if with_ln else None,
                          ln_b=ln_b.to(DEV) if with_ln else None, err_flag=err.t, **kw)
            x.check(want, "embed_ln_kernel x " + what)
            err.check(torch.tensor([flag], dtype=I32), "embed_ln_kernel err_flag " + what)
            if not with_ln:
                xn.check(ops.poison(M * C), "embed_ln_kernel without weights leaves xn alone")
                continue
            xn.pads_intact("xn")
            got = xn.cpu(F32).view(M, C)
            assert torch.equal(bits(got[~real]), bits(ln_b.expand(M, C)[~real])), "xn of a zero row is ln_b"
            d = float(np.abs(got.double().numpy() - U.ln64(want.numpy(), ln_w.numpy(), ln_b.numpy()))[real.numpy()].max()) if real.any() else 0.0
            print(f"OBSERVED embed_ln_kernel xn {what}: vs ln64 {d:.3e}")
            assert d <= U.TOL, f"embed_ln_kernel xn {what}: {d:.3g} off ln64 (bound {U.TOL})"


# ---- the qkv0 table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,dh", [(64, 32), (512, 64), (1024, 128), (512, 128)])
@pytest.mark.parametrize("paging", ["arith", "table"])
def test_qkv0_table_row(C, dh, paging):
    """embed_qkv0_row through embed_qkv0_kernel, argmax_advance_embed_kernel and the fused sampler tail: x, qkv = the table row, K | V
    in layer 0's page at the row's next ctx_len (0, 63, 64, 127; 64 * max_pages is beyond the table: nothing cached, x and qkv still
    written), no statistics; a parked row writes at its parked length"""
    max_pages = 2
    # (done, len): finished and parked rows stay at len, running rows move to len + 1
    spec = [(1, 0), (1, 63), (2, 64), (1, 127), (1, 128), (0, 62), (0, 63), (0, 126), (0, 127), (2, 0)]
    B = len(spec)
    table = dict(n_head=C // dh, head_dim=dh, max_pages=max_pages, arith_batch=B + 3 if paging == "arith" else 0,
                 n_pages=max_pages * (B + 3) if paging == "arith" else 23)
    sc = dict(tok=(np.arange(B) * 5 + 3) % VOCAB, step=np.zeros(B, np.int64), fed=(np.arange(B) * 11 + 40) % (VOCAB + 5),
              len=np.asarray([l for _, l in spec]), done=np.asarray([d for d, _ in spec]), eos=np.full(B, -1), max_new=np.zeros(B, np.int64),
              cap=np.full(B, U.NONE))
    ex = U.expected_state(sc, True)
    assert sorted(set(ex["next_len"].tolist())) == [0, 63, 64, 127, 128]
    lg = small_logits(B, VOCAB)
    lg[torch.arange(B), torch.from_numpy(sc["tok"])] = U.WIN
    for kind in (_lib.TAIL_ARGMAX_EMBED, _lib.TAIL_SAMPLE):
        st, sampled, em = State(sc), Buf.poison(B, I32), Embed(B, C, absolute_pos=1, table=table, seed=C + dh)
        extra = dict(partials=planted_partials(sc["tok"])) if kind == _lib.TAIL_ARGMAX_EMBED else dict(sampler=dict(logits=lg.to(DEV)))
        ops.step_tail(kind, B, st.args(), rows=records(sc)[0], sampled=sampled.t, **extra, **em.args())
        st.check(ex, f"kind {kind} table form")
        em.check(ex["fed"], ex["next_len"], f"kind {kind} C={C} dh={dh} {paging}")
    # embed_qkv0_kernel: ids = cur_ids at ctx_len, no bookkeeping; ids outside the vocabulary are clamped and flagged
    em, err = Embed(B, C, absolute_pos=1, table=table, seed=C + dh), Buf(torch.zeros(1, dtype=I32))
    cur, ctx = Buf(i32(ex["fed"])), Buf(i32(ex["next_len"]))
    ops.step_tail(_lib.TAIL_EMBED_QKV0, B, dict(cur_ids=cur.t, ctx_len=ctx.t, n_steps=0), err_flag=err.t, **em.args())
    cur.check(i32(ex["fed"]), "embed_qkv0_kernel reads cur_ids")
    ctx.check(i32(ex["next_len"]), "embed_qkv0_kernel reads ctx_len")
    em.check(ex["fed"], ex["next_len"], f"embed_qkv0_kernel C={C} dh={dh} {paging}")
    err.check(torch.tensor([int(any(not 0 <= f < VOCAB for f in ex["fed"]))], dtype=I32), "embed_qkv0_kernel err_flag")
    assert any(not 0 <= f < VOCAB for f in ex["fed"])


# ---- refusals: on the host, before any launch ----------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """B > 512, C % 4 != 0, C > 4096 and the table form's cases (C > 1024, fp16 pages, C % head_dim != 0, no qkv): RuntimeError with
    every output still poison"""
    def attempt(kind, B, C, table=None, drop_qkv=False, what=""):
        sc = finished_rows([1] * B, [1] * B)
        st, sampled = State(sc), Buf.poison(B, I32)
        x, stats = Buf.poison((B + 63) // 64 * 64 * ((C + 31) // 32 * 32)), Buf.poison(4 * B)   # room for whatever a launch would write
        tok_emb, pos_emb = torch.zeros(VOCAB * C, device=DEV), torch.zeros(POS_ROWS * C, device=DEV)
        kw = dict(embed=dict(tok_emb=tok_emb, pos_emb=pos_emb, x=x.t, stats=stats.t, C=C, vocab=VOCAB, pos_rows=POS_ROWS, absolute_pos=0))
        outs = [x, stats, sampled]
        if table:
            H, dh, dt = table
            qkv, pages = Buf.poison(B * 3 * C), Buf.poison(ops.kv_page_elems(2 * B, H, dh), dt)
            kw["table"] = dict(qkv0=torch.zeros(VOCAB * 3 * C, device=DEV), qkv=None if drop_qkv else qkv.t, pages=pages.t, n_pages=2 * B, n_head=H,
                               head_dim=dh, page_table=torch.zeros(B, 2, dtype=I32, device=DEV), arith_batch=0)
            outs += [qkv, pages]
        lg = small_logits(B, VOCAB).to(DEV)
        extra = dict(partials=planted_partials(sc["tok"])) if kind == _lib.TAIL_ARGMAX_EMBED else \
            dict(sampler=dict(logits=lg)) if kind == _lib.TAIL_SAMPLE else {}
        before = [o.full.cpu().clone() for o in outs]
        with pytest.raises(RuntimeError):
            ops.step_tail(kind, B, st.args(), rows=records(sc)[0], sampled=sampled.t, **extra, **kw)
        for o, was in zip(outs, before):
            assert torch.equal(o.full.cpu(), was), f"{what}: a refused call wrote something"
        st.check(dict(cur_ids=sc["fed"], ctx_len=sc["len"], done=sc["done"], row_step=sc["step"], n_done=0,
                      ids_out=np.full((B, U.N_STEPS), U.POISON)), what + ": a refused call moved the state")
    for kind in (_lib.TAIL_ARGMAX_EMBED, _lib.TAIL_SAMPLE):
        attempt(kind, 4, 6, what="C % 4 != 0")
        attempt(kind, 4, 4100, what="C > 4096")
        attempt(kind, 513, 32, what="B > 512")
        attempt(kind, 65, 1028, what="k-tiled x: C % 32 != 0 with more than 64 rows")
        attempt(kind, 65, 4, what="k-tiled x: C = 4 with more than 64 rows")
        attempt(kind, 4, 2048, table=(32, 64, F32), what="table: C > 1024")
        attempt(kind, 4, 64, table=(2, 32, torch.float16), what="table: fp16 pages")
        attempt(kind, 4, 64, table=(1, 48, F32), what="table: C % head_dim != 0")
        attempt(kind, 4, 64, table=(2, 32, F32), drop_qkv=True, what="table: no qkv")
    attempt(_lib.TAIL_EMBED_QKV0, 4, 64, what="embed_qkv0 without a table")
    attempt(_lib.TAIL_EMBED_QKV0, 4, 64, table=(2, 32, torch.float16), what="embed_qkv0: fp16 pages")
    sc = finished_rows([1] * 513, [1] * 513)
    for kind in (_lib.TAIL_ARGMAX, _lib.TAIL_ADVANCE):
        st, sampled = State(sc), Buf(i32(sc["tok"]))
        with pytest.raises(RuntimeError):
            ops.step_tail(kind, 513, st.args(), partials=planted_partials(sc["tok"]), sampled=sampled.t)
        st.row_step.check(i32(sc["step"]), "B > 512 moved row_step")
    a = _lib.StepTailArgs(kind=0, B=1, reserved=1)
    assert _lib.load().mgea_op_step_tail(a, None) == _lib.EINVAL
    # embed_stats_kernel: the same k-tiled limit
    ids = torch.zeros(65, 1, dtype=I32, device=DEV)
    for C in (1028, 4):
        x, stats = Buf.poison(128 * ((C + 31) // 32 * 32)), Buf.poison(4 * 65)
        with pytest.raises(RuntimeError):
            ops.dec_embed(0, ids, torch.zeros(VOCAB, C, device=DEV), torch.zeros(POS_ROWS, C, device=DEV), x.t, stats.t)
        x.check(ops.poison(x.n), f"embed_stats_kernel C={C} with 65 rows: refused, nothing written")
        stats.check(ops.poison(4 * 65), "stats")


# ---- budgets and parking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 256, 257])
def test_fill_sampler_params(B):
    cfg = dict(temperature=0.75, top_k=13, top_p=0.5, eos_id=9, seed=(7 << 32) | 5)
    recs = ops.row_budgets(B, 4, config=cfg)
    for b, r in enumerate(recs):
        assert r == dict(temperature=0.75, top_k=13, top_p=0.5, penalty=1.0, eos_id=9, max_new=U.NONE, seed=(7 << 32) | 5, stream=b, ctx_cap=U.NONE), (b, r)


def test_clamp_budgets():
    """max_new = min(max_new, reserved - len) with len clamped to [1, T], ctx_cap = reserved; lens NULL; a row exactly at the limit"""
    B, T, R = 259, 6, 10
    rs = np.random.RandomState(1)
    budgets = rs.randint(0, 12, size=B)              # 0 = no budget
    lens = rs.randint(-2, T + 4, size=B)
    lens[:4], budgets[:4] = [6, 6, 1, 0], [4, 5, 9, 0]   # exactly at the limit, one over, the longest room, len clamped up to 1
    rows = [RowSampling(1.0, 1, None, None, -1, int(m), 0) for m in budgets]
    for use_lens in (True, False):
        recs = ops.row_budgets(B, T, rows=rows, lens=i32(lens).to(DEV) if use_lens else None, reserved=R)
        for b, r in enumerate(recs):
            n = min(max(int(lens[b]), 1), T) if use_lens else T
            assert (r["max_new"], r["ctx_cap"], r["stream"]) == (min(int(budgets[b]) or U.NONE, R - n), R, b), (b, r, n)
    recs = ops.row_budgets(B, T, rows=rows, reserved=0)
    assert all(r["ctx_cap"] == U.NONE and r["max_new"] == (int(m) or U.NONE) for r, m in zip(recs, budgets))
    for T_bad in (R, R + 1):
        with pytest.raises(RuntimeError):
            ops.row_budgets(B, T_bad, rows=rows, reserved=R)


def test_unpark_rows():
    B = 259
    done = np.arange(B) % 3
    ctx = 5 + np.arange(B) % 7
    d, c = Buf(i32(done)), Buf(i32(ctx))
    ops.unpark_rows(d.t, c.t, B)
    d.check(i32(np.where(done == 2, 1, done)), "unpark: done 2 -> 1, 0 and 1 untouched")
    c.check(i32(np.where(done == 2, ctx + 1, ctx)), "unpark: ctx_len + 1 for the parked rows only")
    d2, c2 = Buf(i32(done)), Buf(i32(ctx))
    ops.unpark_rows(d2.t, c2.t, 256)                       # rows beyond B are not touched
    d2.check(i32(np.where((done == 2) & (np.arange(B) < 256), 1, done)), "unpark: B bounds the launch")


def test_clamp_park_unpark_chain():
    """add_lens, clamp, steps until a row parks, more steps (the parked row moves only row_step and -1 entries), unpark: the chain ends
    where the rule ends"""
    B, T, R, n_steps = 4, 4, 8, 7
    lens = [4, 2, 3, 1]
    asked = [0, 3, 0, 2]
    ctx = Buf(torch.zeros(B, dtype=I32))
    ops.add_lens(ctx.t, i32(lens).to(DEV), T, B)
    ctx.check(i32(lens), "add_lens")
    recs = ops.row_budgets(B, T, rows=[RowSampling(1.0, 1, None, None, -1, m, 0) for m in asked], lens=i32(lens).to(DEV), reserved=R)
    assert [(r["max_new"], r["ctx_cap"]) for r in recs] == [(4, 8), (3, 8), (5, 8), (2, 8)]
    rows = [RowSampling(1.0, 1, None, None, -1, r["max_new"], 0) for r in recs]
    caps = [r["ctx_cap"] for r in recs]
    sc = dict(fed=np.asarray([9, 9, 9, 9]), len=np.asarray(lens), done=np.zeros(B, np.int64), step=np.zeros(B, np.int64), tok=np.zeros(B, np.int64))
    st = State(sc, n_steps=n_steps)
    model = [dict(fed=9, len=lens[b], done=0, step=0) for b in range(B)]
    want_ids = np.full((B, n_steps), U.POISON, np.int64)
    n_done, parked_at = 0, None
    for t in range(n_steps):
        toks = [10 + 4 * t + b for b in range(B)]
        ops.step_tail(_lib.TAIL_ADVANCE, B, st.args(), rows=rows, ctx_cap=caps, sampled=i32(toks).to(DEV))
        for b, m in enumerate(model):
            r = U.end_of_step(toks[b], m["step"], m["fed"], m["len"], m["done"], -1, recs[b]["max_new"], caps[b], n_steps)
            if r.entry is not None:
                want_ids[b, m["step"]] = r.entry
            if m["done"] == 2:
                assert (r.cur_id, r.ctx_len, r.done) == (m["fed"], m["len"], 2), "a parked row moves nothing but row_step"
            m.update(fed=r.cur_id, len=r.ctx_len, done=r.done, step=r.row_step)
            n_done += r.n_done
            if r.done == 2 and parked_at is None:
                parked_at = t
        st.check(dict(cur_ids=[m["fed"] for m in model], ctx_len=[m["len"] for m in model], done=[m["done"] for m in model],
                      row_step=[m["step"] for m in model], n_done=n_done, ids_out=want_ids), f"chain step {t}")
    assert parked_at == 3 and [m["done"] for m in model] == [2, 1, 2, 1] and model[0]["len"] == R - 1 and n_done == B
    ops.unpark_rows(st.done.t, st.ctx_len.t, B)
    st.done.check(i32([1, 1, 1, 1]), "unpark")
    st.ctx_len.check(i32([R, 5, 8, 3]), "the unparked row holds all its tokens: ctx_len = the reservation")


# ---- take_last / add_lens ---------------------------------------------------------------------------------------------------------
def test_take_last_and_add_lens():
    B, T = 259, 5
    ids = (np.arange(B * T).reshape(B, T) * 13 + 1) % 1000
    lens = np.asarray([1, T, 0, T + 3, -4, 3][: 6] * 44)[:B]
    for use in (True, False):
        n = np.clip(lens, 1, T) if use else np.full(B, T)
        cur = Buf.poison(B, I32)
        ops.take_last(i32(ids).to(DEV), i32(lens).to(DEV) if use else None, cur.t)
        cur.check(i32(ids[np.arange(B), n - 1]), f"take_last lens={'given' if use else 'NULL'}")
        ctx = Buf(i32(np.arange(B) % 11))
        ops.add_lens(ctx.t, i32(lens).to(DEV) if use else None, T, B)
        ctx.check(i32(np.arange(B) % 11 + (lens if use else T)), f"add_lens lens={'given' if use else 'NULL'} (unclamped)")
    ctx = Buf(i32(np.zeros(B)))
    ops.add_lens(ctx.t, None, T, 256)
    ctx.check(i32(np.where(np.arange(B) < 256, T, 0)), "add_lens: B bounds the launch")


# ---- ids_out == NULL ---------------------------------------------------------------------------------------------------------------
def test_every_caller_without_ids_out():
    """ids_out is optional (a single step has no history): every caller leaves the same state and writes no entry anywhere"""
    B = 64
    sc = U.scenarios(B, True)
    ex = U.expected_state(sc, True)
    rows, caps = records(sc)
    part = planted_partials(sc["tok"])
    lg = small_logits(B, VOCAB)
    lg[torch.arange(B), torch.from_numpy(sc["tok"])] = U.WIN
    for kind in (_lib.TAIL_ARGMAX, _lib.TAIL_ARGMAX_EMBED, _lib.TAIL_ADVANCE, _lib.TAIL_SAMPLE):
        st = State(sc, ids_out=False)
        sampled = Buf(i32(sc["tok"])) if kind == _lib.TAIL_ADVANCE else Buf.poison(B, I32)
        em = Embed(B, 128) if kind in (_lib.TAIL_ARGMAX_EMBED, _lib.TAIL_SAMPLE) else None
        extra = dict(partials=part) if kind in (_lib.TAIL_ARGMAX, _lib.TAIL_ARGMAX_EMBED) else \
            dict(sampler=dict(logits=lg.to(DEV))) if kind == _lib.TAIL_SAMPLE else {}
        ops.step_tail(kind, B, st.args(), rows=rows, ctx_cap=caps, sampled=sampled.t, **extra, **(em.args() if em else {}))
        st.check(ex, f"kind {kind} without ids_out")
        sampled.check(i32(sc["tok"]), f"kind {kind} without ids_out: sampled")
        if em:
            em.check(ex["fed"], ex["next_len"], f"kind {kind} without ids_out")
