"""Host code shared by the causal-mode tests (test_causal_host.py on the CPU; test_gpu_causal_attention.py, test_gpu_causal_engine.py).

CausalRef        a torch-CPU fp32 restatement of the causal mode (MGEA_POS_CAUSAL) as three switches on top of oracle/decoder_ref.py:
                   true_pos     the token at index p of a row gets pos_emb[p] (clamped to the table's last row), not pos_emb[:T] per call;
                   causal_mask  position i attends positions <= i (ragged rows by validity, as before);
                   feed_once    generate_greedy prefills p[:-1] and feeds p[-1] first, instead of caching p[-1] twice.
                 With all three off every operation is DecoderRef's, in its order: bit-equal results (test_causal_host.py), which ties
                 this restatement to the golden-pinned oracle.
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
