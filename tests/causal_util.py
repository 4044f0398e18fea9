"""Host code shared by the causal-mode tests (test_causal_host.py on the CPU; test_gpu_causal_attention.py, test_gpu_causal_engine.py).

CausalRef        a torch-CPU fp32 restatement of the causal mode (MGEA_POS_CAUSAL) as three switches on top of oracle/decoder_ref.py:
                   true_pos     the token at index p of a row gets pos_emb[p] (clamped to the table's last row), not pos_emb[:T] per call;
                   causal_mask  position i attends positions <= i (ragged rows by validity, as before);
                   feed_once    generate_greedy prefills p[:-1] and feeds p[-1] first, instead of caching p[-1] twice.
                 With all three off every operation is DecoderRef's, in its order: bit-equal results (test_causal_host.py), which ties
                 this restatement to the golden-pinned oracle.
causal_step_logits, walk
                 the generation forms on top of CausalRef.forward: every prompt prefilled without its last token, that token fed
                 first, then the generated (or forced) ids; the processing of a step is assembled from the host rules the reference-mode
                 tests use (class_penalty_util.host_rule, penalize, TokenGrammar, the guidance and blend mixes), none of them restated.
                 form_case names the cases test_causal_host.py qualifies on the CPU and test_gpu_causal_forms.py runs.
input families   attention inputs whose causal answer is known in closed form, each held to fp64 causal softmax attention at 1e-6 where
                 it is built.  Every value is exact in fp16, so fp16 KV pages hold them.  A query is (row b, index i) at global position
                 past[b] + i; it sees the keys t <= past[b] + i with t < n_keys[b].
                   latest     k[t] = t e_0, q = c e_0 with consecutive keys >= 20 apart in scaled score: out = V[last visible key].  One
                              future key counted gives V[j > i]; the diagonal key lost gives V[i - 1];
                   pointer    test_gpu_attention_exact._family("pointer") with the targets restricted to visible keys: 0, both ends of
                              every 64-key tile at or below the query, and the query's own position;
                   histogram  q = 0, V[t] = e_(t mod dh): out[d] * (visible keys) = the visible t with t mod dh == d.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle.decoder_ref import DecoderRef
from test_gpu_attention_exact import _family, _v_rows

FAMILIES = ("latest", "pointer", "histogram")
TOL_F32 = 2e-5            # the fp32 bound of the exact-answer attention tests


# ---- the restated model ---------------------------------------------------------------------------------------------------------
class CausalRef(DecoderRef):
    def __init__(self, state_dict, n_head: int = 8, true_pos: bool = True, causal_mask: bool = True, feed_once: bool = True):
        super().__init__(state_dict, n_head)
        self.true_pos, self.causal_mask, self.feed_once = true_pos, causal_mask, feed_once

    def _attend_allowed(self, q, k, v, allowed):
        """q [B,Tq,C], k/v [B,Tk,C], allowed [B,Tq,Tk] bool -> [B,Tq,C]; a query that may see nothing gives a zero row"""
        B, Tq, C = q.shape
        Tk = k.shape[1]
        H, dh = self.H, self.dh
        q = q.view(B, Tq, H, dh).transpose(1, 2)
        k = k.view(B, Tk, H, dh).transpose(1, 2)
        v = v.view(B, Tk, H, dh).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh))
        s = s.masked_fill(~allowed[:, None, :, :], float("-inf"))
        p = torch.softmax(s, dim=-1)
        p = torch.where(allowed.any(-1)[:, None, :, None], p, torch.zeros_like(p))
        return (p @ v).transpose(1, 2).reshape(B, Tq, C)

    @torch.no_grad()
    def forward(self, idx, cache=None, cache_valid=None, new_valid=None):
        """DecoderRef.forward's signature and returns.  The cache is padded per row (ragged prompts): a row's position counts its
        valid cached tokens, and a new token sees every valid cached token and the valid new tokens up to itself."""
        B, T = idx.shape
        C = self.C
        if cache is None:
            cache = [None] * self.NL
        if new_valid is None:
            new_valid = torch.ones(B, T, dtype=torch.bool)
        if cache[0] is not None and cache_valid is None:
            cache_valid = torch.ones(B, cache[0][0].shape[1], dtype=torch.bool)
        if self.true_pos:
            past = cache_valid.sum(1) if cache[0] is not None else torch.zeros(B, dtype=torch.long)
            pos = (past[:, None] + torch.arange(T)[None, :]).clamp(max=self.seq_len - 1)
            x = self.tok_emb[idx] + self.pos_emb[pos]
        else:
            if T > self.seq_len:
                raise RuntimeError(f"T={T} exceeds the position table ({self.seq_len} rows) (api_cache.py:99)")
            x = self.tok_emb[idx] + self.pos_emb[:T]
        valid = new_valid if cache[0] is None else torch.cat([cache_valid, new_valid], 1)
        mask = None if bool(valid.all()) else valid
        Tc = valid.shape[1] - T
        if self.causal_mask:   # [B, T, Tc + T]: the cache whole, the new tokens up to the query
            tri = torch.ones(T, T, dtype=torch.bool).tril()
            allowed = torch.cat([torch.ones(T, Tc, dtype=torch.bool), tri], 1)[None] & valid[:, None, :]
        presents = []
        for L, past_kv in zip(self.layers, cache):
            xn = F.layer_norm(x, (C,), L["n1_w"], L["n1_b"], 1e-5)
            qkv = xn @ L["in_w"].t() + L["in_b"]
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
            if self.causal_mask:   # (slots of no token: zeros, so that a row without any valid token leaves no NaN behind)
                k = torch.where(new_valid[..., None], k, torch.zeros_like(k))
                v = torch.where(new_valid[..., None], v, torch.zeros_like(v))
            if past_kv is not None:
                k = torch.cat([past_kv[0], k], 1)
                v = torch.cat([past_kv[1], v], 1)
            presents.append((k, v))
            a = self._attend_allowed(q, k, v, allowed) if self.causal_mask else self._attend(q, k, v, mask)
            x = x + (a @ L["out_w"].t() + L["out_b"])
            h = F.layer_norm(x, (C,), L["n2_w"], L["n2_b"], 1e-5)
            h = F.gelu(h @ L["l1_w"].t() + L["l1_b"])
            x = x + (h @ L["l2_w"].t() + L["l2_b"])
        logits = x @ self.head_w.t() + self.head_b
        return logits, presents, valid

    @staticmethod
    def prefill_lens(lens: Sequence[int], feed_once: bool = True) -> List[int]:
        """the host rule of the engine's gen_prefill: the tokens of each prompt that are prefilled (lens_m1)"""
        return [max(int(n), 1) - 1 if feed_once else int(n) for n in lens]

    @torch.no_grad()
    def generate_greedy(self, prompts, n_steps: int, return_logits: bool = False):
        """DecoderRef.generate_greedy's signature and returns.  feed_once: the prefill takes every prompt without its last token (a
        prompt of one token prefills nothing; a batch of them runs no prefill at all) and the first step feeds that token."""
        B = len(prompts)
        pre = self.prefill_lens([len(p) for p in prompts], self.feed_once)
        Tp = max(pre)
        cache, cvalid = None, None
        if Tp > 0:
            idx = torch.zeros(B, Tp, dtype=torch.long)
            valid = torch.zeros(B, Tp, dtype=torch.bool)
            for b, p in enumerate(prompts):
                idx[b, :pre[b]] = torch.tensor(list(p[:pre[b]]), dtype=torch.long)
                valid[b, :pre[b]] = True
            _, cache, cvalid = self.forward(idx, None, None, valid)
        last = torch.tensor([p[-1] for p in prompts]).view(B, 1)
        outs = [list(p) for p in prompts]
        step_logits = []
        for _ in range(n_steps):
            logits, cache, cvalid = self.forward(last, cache, cvalid, None)
            lg = logits[:, -1, :]
            if return_logits:
                step_logits.append(lg.clone())
            last = lg.argmax(-1, keepdim=True)
            for b in range(B):
                outs[b].append(int(last[b, 0]))
        if return_logits:
            return outs, torch.stack(step_logits, 1)
        return outs


def diagnose_greedy(eng, ref: CausalRef, prompts, n_steps: int, got: List[List[int]], label: str) -> None:
    """Strict comparison of greedy ids with CausalRef's, in the style of parity_util: on a difference, say where and how wide the
    reference's top-2 gap is there, then fail.  (parity_util's own teacher-forced diagnosis assumes the re-fed token.)"""
    want, sl = ref.generate_greedy(prompts, n_steps, return_logits=True)
    srt = sl.sort(-1).values
    gap = srt[..., -1] - srt[..., -2]
    bad = []
    for b, p in enumerate(prompts):
        w = want[b][len(p):]
        if got[b] != w:
            s = next(i for i in range(n_steps) if got[b][i] != w[i])
            bad.append(f"row {b} (prompt of {len(p)}) step {s}: engine {got[b][s]} vs reference {w[s]}, reference top-2 gap {float(gap[b, s]):.3e}")
    assert not bad, f"{label}: greedy ids differ from CausalRef: " + "; ".join(bad)


# ---- the input families ---------------------------------------------------------------------------------------------------------
def ref64_causal(q, k, v, n_keys, past):
    """fp64 causal softmax attention: q [B, Tq, H, dh], k / v [B, L, H, dh]; query (b, i) sees t <= past[b] + i, t < n_keys[b].
    A query that sees nothing gives zeros."""
    B, Tq, H, dh = q.shape
    L = k.shape[1]
    out = np.zeros(q.shape)
    for b in range(B):
        s = (q[b].transpose(1, 0, 2) @ k[b].transpose(1, 2, 0)) / math.sqrt(dh)             # [H, Tq, L]
        see = (np.arange(L)[None, :] <= past[b] + np.arange(Tq)[:, None]) & (np.arange(L)[None, :] < n_keys[b])
        s = np.where(see[None], s, -np.inf)
        mx = np.where(see.any(-1), s.max(-1), 0.0)
        p = np.where(see[None], np.exp(s - mx[..., None]), 0.0)
        den = np.where(see.any(-1)[None], p.sum(-1), 1.0)
        out[b] = ((p / den[..., None]) @ v[b].transpose(1, 0, 2)).transpose(1, 0, 2)
    return out


def _exact_f16(x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return bool((t.half().double() == t).all())


class CausalCase:
    """One launch: q [B, Tq, H, dh], k, v [B, L, H, dh], exp [B, Tq, H, dh] (fp64); rows [B, Tq]: the queries that exist (their
    position lies inside the row); n_keys [B], past [B]."""

    def __init__(self, family, n_keys, past, Tq, H, dh):
        n_keys, past = np.asarray(n_keys), np.asarray(past)
        B, L = len(n_keys), max(int(n_keys.max()), 1)
        self.family, self.n_keys, self.past, self.H, self.dh = family, n_keys, past, H, dh
        pos = past[:, None] + np.arange(Tq)[None, :]                       # [B, Tq]
        self.rows = pos < n_keys[:, None]
        last = np.clip(np.minimum(pos, n_keys[:, None] - 1), 0, None)      # the last visible key (an empty row: key 0, never checked)
        valid = np.arange(L)[None, :] < np.where(n_keys > 0, n_keys, L)[:, None]     # (an empty row is built as a full one)
        if family == "latest":
            c = 2.0 ** math.ceil(math.log2(20.0 * math.sqrt(dh)))
            q = np.zeros((B, Tq, H, dh)); q[..., 0] = c
            k = np.zeros((B, L, H, dh)); k[..., 0] = np.arange(L)[None, :, None]
            v = _v_rows(B, L, H, dh)
            exp = np.stack([v[b, last[b]] for b in range(B)])
        elif family == "pointer":
            tg = []
            for b in range(B):
                per_h = []
                for h in range(H):
                    row = []
                    for i in range(Tq):
                        e = int(last[b, i])
                        cand = [0, e] + [t for j in range(0, e + 1, 64) for t in (j, j + 63) if t <= e]
                        cand = list(dict.fromkeys(cand))
                        row.append(cand[(i + 3 * h) % len(cand)])
                    per_h.append(row)
                tg.append(per_h)
            q, k, v, exp = _family("pointer", valid, H, dh, Tq=Tq, q_targets=tg)
        else:
            assert family == "histogram"
            q = np.zeros((B, Tq, H, dh))
            k = np.zeros((B, L, H, dh)); k[..., 1] = (np.arange(L) % 7)[None, :, None] - 3.0      # (any key: q = 0)
            v = np.zeros((B, L, H, dh))
            exp = np.zeros((B, Tq, H, dh))
            for b in range(B):
                for h in range(H):
                    hot = (np.arange(L) + 3 * h + 5 * b) % dh
                    v[b, np.arange(L), h, hot] = 1.0
                    for i in range(Tq):
                        n = int(last[b, i]) + 1
                        exp[b, i, h] = np.bincount(hot[:n], minlength=dh) / n
        assert _exact_f16(q) and _exact_f16(k) and _exact_f16(v), "inputs must be exact in fp16"
        self.q, self.k, self.v, self.exp = q, k, v, exp
        err = np.abs(ref64_causal(q, k, v, n_keys, past) - exp)[self.rows]
        err = float(err.max()) if err.size else 0.0
        assert err < 1e-6, f"{family}: the closed form is {err:.2e} off fp64 causal softmax attention"

    def qkv(self):
        """dense [B, T, 3 C] fp32 (self-attention: Tq == L, past == 0)"""
        B, T = self.q.shape[:2]
        assert T == self.k.shape[1] and not self.past.any()
        return torch.from_numpy(np.concatenate([x.reshape(B, T, -1) for x in (self.q, self.k, self.v)], -1)).float()

    def check(self, out, what=""):
        """out [B, Tq, C] fp32 from a kernel: the existing queries against the closed form (2e-5: absolute, histogram relative), every
        other query of a row WITHOUT keys a zero row"""
        got = out.detach().double().cpu().numpy().reshape(self.exp.shape)
        tol = TOL_F32 * self.exp if self.family == "histogram" else np.full(self.exp.shape, TOL_F32)
        bad = ~(np.abs(got - self.exp) <= tol) & self.rows[:, :, None, None]
        if bad.any():
            b, i, h, d = (int(x[0]) for x in np.nonzero(bad))
            raise AssertionError(f"{self.family} {what}: {int(bad.sum())} wrong outputs; first at row {b} query {i} head {h} dim {d}: "
                                 f"got {got[b, i, h, d]!r}, expected {self.exp[b, i, h, d]!r} +- {tol[b, i, h, d]:.2e}")


# ---- the shapes of the GPU tests (test_causal_host.py builds every one of them on the CPU) ----------------------------------------
DENSE_T = [1, 2, 63, 64, 65, 127, 128, 129, 200, 300]
DENSE_DH = [32, 64, 96]
DENSE_B, DENSE_H = 4, 3


def dense_lens(kind, T):
    """None, or ragged lengths with 0 and 1 among them"""
    return None if kind == "none" else [T, 0, 1, max(1, T - 1)]


@functools.lru_cache(maxsize=None)
def dense_case(family, kind, T, dh):
    lens = dense_lens(kind, T)
    return CausalCase(family, [T] * DENSE_B if lens is None else lens, [0] * DENSE_B, T, DENSE_H, dh)


PAGED_CTX = [(0, 1, 63, 64), (65, 200, 0, 64)]            # ragged across the rows; 0, 1, 63, 64, 65, 200 all occur
PAGED_T = [2, 5, 64, 70]
PAGED_DH = [32, 64, 96, 128]                             # every head_dim the paged launcher has (fp16 pages: 32, 64, 128)
PAGED_B, PAGED_H = 4, 2


def paged_lens(T):
    """ragged new-token counts: a full row, one token, a padded tail"""
    return [T, 1, max(1, T - 1), max(1, T // 2)]


@functools.lru_cache(maxsize=None)
def paged_case(family, ctx, T, dh):
    lens = paged_lens(T)
    return CausalCase(family, [c + n for c, n in zip(ctx, lens)], list(ctx), T, PAGED_H, dh)


# ---- the generation forms on the causal oracle ------------------------------------------------------------------------------------
F32_TOL = 2e-4            # what the fp32 engine is held to against CausalRef (test_gpu_causal_engine.py)
FORM_LENS = (1, 2, 5, 65)
FORM_STEPS = 16
FORM_EOS = 2
FORM_TEMPERATURE = 0.8
NINF = -math.inf


class CausalSteps:
    """CausalRef.generate_greedy's loop one step at a time and one row at a time (B = 1 calls of CausalRef.forward: no padding, so with
    the three switches off a row is DecoderRef's own loop, bit for bit).  Every prompt is prefilled without its last token (a prompt of
    one token prefills nothing); `first` holds the last tokens, which the first feed() takes."""

    def __init__(self, ref: CausalRef, prompts):
        self.ref = ref
        self.rows = []
        for p in prompts:
            n = ref.prefill_lens([len(p)], ref.feed_once)[0]
            cache = valid = None
            if n > 0:
                _, cache, valid = ref.forward(torch.tensor([list(p[:n])], dtype=torch.long))
            self.rows.append([cache, valid])
        self.first = [int(p[-1]) for p in prompts]

    def feed(self, ids) -> torch.Tensor:
        """feed ids[b] to row b: fp32 [B, V], the logits that choose each row's next token"""
        out = []
        for row, t in zip(self.rows, ids):
            lg, row[0], row[1] = self.ref.forward(torch.tensor([[int(t)]], dtype=torch.long), row[0], row[1])
            out.append(lg[0, -1])
        return torch.stack(out)


def causal_step_logits(ref: CausalRef, prompts, fed) -> torch.Tensor:
    """fp32 [B, n, V], n = len(fed[b]): entry s is the logits that choose generated token s of a row that generated fed[b][0 .. s-1] --
    the prompt without its last token prefilled, the last token fed, then fed[b][0 .. n-2]."""
    n = len(fed[0])
    assert all(len(f) == n for f in fed)
    steps = CausalSteps(ref, prompts)
    cur, out = steps.first, []
    for s in range(n):
        out.append(steps.feed(cur))
        cur = [f[s] for f in fed]
    return torch.stack(out, 1)


@dataclasses.dataclass
class Form:
    """what a generation does to a row's logits between the model and the draw, in the order of include/mgea.h: (the mix of a pair or a
    group,) class penalty, repetition penalty, bias, grammar mask, the EOS ban of min_new_tokens, temperature"""
    penalty: Optional[float] = None
    bias: Optional[np.ndarray] = None          # [B, V]
    eos: Optional[Sequence[int]] = None        # per row, -1: none
    min_new: Optional[Sequence[int]] = None
    grammar: object = None                     # a TokenGrammar, with starts
    starts: Optional[Sequence[int]] = None
    class_of: Optional[np.ndarray] = None      # with cpen: (frequency, presence, window) per row
    cpen: Optional[Sequence] = None
    temperature: float = 1.0


def mix_weight(w) -> float:
    """the sum of the absolute mix weights of a row: 1 when it is not mixed"""
    return float(sum(abs(v) for v in w))


def walk(ref: CausalRef, groups, weights, n: int, form: Optional[Form] = None, forced=None):
    """n steps of B rows on the causal oracle.  groups[b]: the prompts row b is mixed from with weights[b] -- one prompt (weights[b]
    ignored), a guidance pair [prompt, negative prompt] with (s, 1 - s), or a blend group; every member is prefilled without its own
    last token, feeds that token first and then the row's ids, as the engine's shadow rows and members do.  The row's set of seen ids
    starts as its FIRST prompt, whole; its grammar state as its start state; its class window empty.  forced: None (greedy: the argmax,
    lowest id among equals), B id lists, or f(b, s, x) -> id with x the processed row.
    Returns ids [B][n] (-1 behind a row's EOS), gaps [B, n] (the processed top-2 gap; inf where fewer than two ids are admitted or the
    row has finished), logprobs / choice [B, n] float64 (log-softmax of the row in front of the repetition penalty / of the processed
    row over the temperature, at the id taken), states and seen as they end."""
    from class_penalty_util import host_rule
    from test_repetition_penalty_host import penalize
    form = form or Form()
    B = len(groups)
    flat = [(b, k) for b, g in enumerate(groups) for k in range(len(g))]
    steps = CausalSteps(ref, [groups[b][k] for b, k in flat])
    cur = list(steps.first)
    seen = [set(int(t) for t in g[0]) for g in groups]
    state = [int(v) for v in form.starts] if form.grammar is not None else [-1] * B
    done = [False] * B
    hist = np.full((B, n), -1, np.int64)
    ids = [[] for _ in range(B)]
    gaps, lp, ch = np.full((B, n), np.inf), np.zeros((B, n)), np.zeros((B, n))
    for s in range(n):
        lg = steps.feed(cur)
        rows = []
        for b, g in enumerate(groups):
            mine = [lg[i].double() for i, (bb, _) in enumerate(flat) if bb == b]
            if len(mine) == 1:
                rows.append(mine[0])
            elif len(mine) == 2:      # test_gpu_guidance: s * logp_c + (1 - s) * logp_u
                sc = float(weights[b][0])
                rows.append(sc * torch.log_softmax(mine[0], 0) + (1.0 - sc) * torch.log_softmax(mine[1], 0))
            else:                     # test_gpu_blend: sum_k w_k * logp_k
                rows.append(sum(wk * torch.log_softmax(x, 0) for wk, x in zip(weights[b], mine)))
        x = torch.stack(rows).numpy().astype(np.float32)
        if form.cpen is not None:
            x = host_rule(x, form.class_of, hist, [s] * B, [int(d) for d in done], form.cpen)
        raw = torch.log_softmax(torch.from_numpy(x).double(), 1)
        if form.penalty is not None:
            x = penalize(x, seen, form.penalty)
        if form.bias is not None:
            x = (x + form.bias).astype(np.float32)
        for b in range(B):
            if state[b] >= 0 and not done[b]:
                x[b, ~form.grammar.allowed(state[b])] = NINF
            if form.eos is not None and form.eos[b] >= 0 and form.min_new is not None and s < form.min_new[b]:
                x[b, form.eos[b]] = NINF
        choice = torch.log_softmax(torch.from_numpy(x).double() / form.temperature, 1)
        srt = np.sort(x, 1)
        with np.errstate(invalid="ignore"):
            gaps[:, s] = np.where(np.isfinite(srt[:, -2]) & ~np.array(done), srt[:, -1] - srt[:, -2], np.inf)
        nxt = x.argmax(1)
        for b in range(B):
            if done[b]:
                ids[b].append(-1)
                continue
            t = int(nxt[b])
            if callable(forced):
                t = int(forced(b, s, x[b]))
            elif forced is not None and forced[b][s] >= 0:
                t = int(forced[b][s])
            ids[b].append(t)
            hist[b, s] = t
            lp[b, s], ch[b, s] = float(raw[b, t]), float(choice[b, t])
            seen[b].add(t)
            if state[b] >= 0:
                state[b] = form.grammar.step(state[b], t)
                assert state[b] >= 0, f"row {b} step {s}: id {t} leaves the grammar"
            done[b] = form.eos is not None and form.eos[b] >= 0 and t == form.eos[b]
        cur = [ids[b][s] if ids[b][s] >= 0 else cur[i] for i, (b, _) in enumerate(flat)]
    return dict(ids=ids, gaps=gaps, logprobs=lp, choice=ch, states=state, seen=seen)


def form_prompts(kind: str, seed: int):
    """B = 4 ragged prompts of 1, 2, 5 and 65 ids (the longest crosses a KV page in the prefill); the 5-token prompt's last id occurs
    nowhere else in it"""
    from test_gpu_causal_engine import GEO
    V = GEO[kind]["vocab"]
    rng = np.random.default_rng(seed)
    ps = [[int(v) for v in rng.integers(1, V, n)] for n in FORM_LENS]
    while ps[2][-1] in ps[2][:-1]:
        ps[2][-1] = int(rng.integers(1, V))
    return ps


# The prompt seed of every (geometry, form): the first seed from 0 at which test_causal_host.py's input conditions hold (found by
# running exactly those conditions on the CPU).
FORM_SEEDS = {("tiny", "plain"): 1, ("tiny", "penalty"): 1, ("tiny", "bias"): 0, ("tiny", "grammar"): 0, ("tiny", "guided"): 1,
              ("tiny", "blended"): 2, ("tiny", "cpen"): 0, ("tiny", "composed"): 0,
              ("fused", "plain"): 0, ("fused", "penalty"): 0, ("fused", "bias"): 0, ("fused", "grammar"): 0, ("fused", "guided"): 1,
              ("fused", "blended"): 18, ("fused", "cpen"): 0, ("fused", "composed"): 0}
FORMS = ("plain", "penalty", "bias", "grammar", "guided", "blended", "cpen", "composed")
GREEDY_FORMS = ("plain", "penalty", "bias", "grammar", "guided", "blended")


@functools.lru_cache(maxsize=None)
def form_case(kind: str, name: str, seed: Optional[int] = None):
    """-> (groups, weights, Form) of the named case on geometry `kind`; seed None: FORM_SEEDS"""
    from test_gpu_blend import WEIGHTS
    from test_gpu_causal_engine import GEO
    from test_gpu_class_penalty import map12
    from test_gpu_generate_entry_points import parity_grammar
    from test_gpu_guidance import SCALES
    from test_gpu_logit_bias import make_bias
    V = GEO[kind]["vocab"]
    seed = FORM_SEEDS[kind, name] if seed is None else seed
    prompts = form_prompts(kind, seed)
    B = len(prompts)
    rng = np.random.default_rng(1000 + seed)
    groups, weights, form = [[p] for p in prompts], [(1.0,)] * B, Form()
    if name == "penalty":
        form = Form(penalty=1.2)
    elif name == "bias":      # row 3's EOS is far ahead once the ban of min_new_tokens lifts: it ends the row at step 3, not before
        bias = make_bias(rng, "mixed", (B, V))
        bias[:, FORM_EOS] = 0.5
        bias[3, FORM_EOS] = 30.0
        form = Form(bias=bias, eos=[FORM_EOS] * B, min_new=[3] * B)
    elif name == "grammar":
        form = Form(grammar=parity_grammar(V), starts=[0, 1, 0, 1])
    elif name == "guided":    # a shadow row prefills nothing
        groups = [[p, p[:1]] for p in prompts]
        weights = [(s, 1.0 - s) for s in SCALES + SCALES[1:2]]
    elif name == "blended":   # the second member prefills nothing, the third is a prompt of its own
        groups = [[p, p[:1], [int(v) for v in rng.integers(1, V, 3)]] for p in prompts]
        weights = [WEIGHTS[b % 2] for b in range(B)]
    elif name == "cpen":
        form = Form(class_of=map12(V), cpen=[(0.5, 2.0, 4), (-0.25, 1.0, 4), (1.0, 0.0, 4), (0.5, 2.0, 4)])
    elif name == "composed":  # rows of at least two tokens (the replay prefills them through forward())
        groups, weights = groups[1:], weights[1:]
        form = Form(penalty=1.2, bias=make_bias(rng, "finite", (B - 1, V)), grammar=parity_grammar(V), starts=[1, 0, 1])
    else:
        assert name == "plain", name
    return groups, weights, form


def gap_floor(weights):
    """[B]: the smallest processed top-2 gap at which the GPU tests demand exact greedy ids: 5 x (sum of |mix weights|) x F32_TOL"""
    return np.array([5.0 * mix_weight(w) * F32_TOL for w in weights])


@functools.lru_cache(maxsize=None)
def draw_forced(kind: str, name: str, n: int = FORM_STEPS, seed: Optional[int] = None):
    """the forced ids of a case's teacher-forced run, drawn on the host from the ids the form admits (a finite processed logit), never
    the row's EOS, about half of them ids the row has seen already.  Two are placed: step 0 of the "penalty" case's 5-token row is that
    row's LAST PROMPT id (a bitmap seeded without it moves the choice value by the penalty), and step 0 of every "cpen" row is another
    id of the class of the row's last prompt id (a window that counted the fed prompt token moves it by the presence term).
    Returns (forced [B][n], the walk's result)."""
    from test_gpu_causal_engine import GEO, reference
    groups, weights, form = form_case(kind, name, seed)
    form = dataclasses.replace(form, temperature=FORM_TEMPERATURE)
    rng = np.random.default_rng(77)
    seen = [set(g[0]) for g in groups]

    def pick(b, s, x):
        ok = np.isfinite(x)
        if form.eos is not None and form.eos[b] >= 0:
            ok[form.eos[b]] = False
        last = groups[b][0][-1]
        if s == 0 and name == "penalty" and b == 2:
            t = last
        elif s == 0 and name == "cpen" and form.class_of[last] >= 0:
            t = int(rng.choice(np.flatnonzero(ok & (form.class_of == form.class_of[last]) & (np.arange(len(x)) != last))))
        else:
            old = [i for i in sorted(seen[b]) if ok[i]]
            t = int(rng.choice(old)) if old and rng.random() < 0.5 else int(rng.choice(np.flatnonzero(ok)))
        seen[b].add(t)
        return t

    res = walk(reference(kind), groups, weights, n, form, pick)
    return res["ids"], res


def input_conditions(kind: str, name: str, seed: Optional[int] = None):
    """What the GPU tests of a case assume about its inputs, from the oracle alone: the complaints, none when the case qualifies.
      greedy forms   the processed top-2 gap of the free-running oracle is at least gap_floor at every (row, step): exact ids, no
                     near-tie exemptions;
      penalty        the 5-token row's step-0 choice value moves by at least 10 x ORACLE_TOL when its last prompt id is not in the set;
      guided         the guided log-probability is at least 0.118 (test_gpu_guidance) from the conditional row's plain one at some
                     step of every row whose negative prompt is not its prompt;
      blended        the same against test_gpu_blend.POWER_FLOOR, every row;
      cpen           penalised and plain log-probabilities differ by at least 10 x SCORED_BOUND somewhere (test_gpu_class_penalty)."""
    from test_gpu_blend import POWER_FLOOR
    from test_gpu_causal_engine import reference
    from test_gpu_class_penalty import SCORED_BOUND
    from test_gpu_logprobs import ORACLE_TOL
    from test_repetition_penalty_host import penalize
    ref = reference(kind)
    groups, weights, form = form_case(kind, name, seed)
    bad = []
    if name in GREEDY_FORMS:
        res = walk(ref, groups, weights, FORM_STEPS, form)
        floor = gap_floor(weights)
        for b in range(len(groups)):
            g = float(res["gaps"][b].min())
            if g < floor[b]:
                bad.append(f"{kind} {name}: row {b}: greedy top-2 gap {g:.2e} below {floor[b]:.1e} at step {int(res['gaps'][b].argmin())}")
    if name in ("penalty", "guided", "blended", "cpen"):
        forced, res = draw_forced(kind, name, FORM_STEPS, seed)
        plain = walk(ref, [g[:1] for g in groups], [(1.0,)] * len(groups), FORM_STEPS, None, forced)
        power = np.abs(res["logprobs"] - plain["logprobs"]).max(1)
    if name == "penalty":
        p = groups[2][0]
        x = causal_step_logits(ref, [p], [[forced[2][0]]])[0].numpy()
        with_last, without = (torch.log_softmax(torch.from_numpy(penalize(x, [s], form.penalty)).double() / FORM_TEMPERATURE, 1)[0, p[-1]]
                              for s in (set(p), set(p[:-1])))
        if abs(float(with_last - without)) < 10 * ORACLE_TOL:
            bad.append(f"{kind} penalty: the last prompt id moves the step-0 choice value by only {abs(float(with_last - without)):.3f}")
    if name == "guided":
        bad += [f"{kind} guided: row {b}: power {power[b]:.3f} < 0.118" for b in range(1, len(groups)) if power[b] < 0.118]
    if name == "blended":
        bad += [f"{kind} blended: row {b}: power {power[b]:.3f} < {POWER_FLOOR[weights[b]]}" for b in range(len(groups))
                if power[b] < POWER_FLOOR[weights[b]]]
    if name == "cpen" and power.max() < 10 * SCORED_BOUND:
        bad.append(f"{kind} cpen: power {power.max():.3f} < {10 * SCORED_BOUND:.3f}")
    return bad
