"""The host side of a generation request, no device in it: the per-row records (RowSampling, Truncation, ClassPenalty, RowSchedule),
the host models of what the engine does with them (TokenGrammar, KVWindow), the check_* rules of include/mgea.h as ValueErrors and
the pack_* functions that turn a batch of records into the C arrays of the native call.  mgea.decoder imports every name back:
`from mgea.decoder import X` is where callers find them.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import RowClassPenalty, RowLogits, RowSampler, RowTruncation


def dense_logit_bias(bias, vocab: int):
    """A logit bias as a dense float32 [vocab] vector: a dict id -> bias is packed on the host (ids not named get 0), a host array
    or tensor is converted, a DEVICE tensor is returned as it is (float32, contiguous).  -inf bans an id.  None stays None."""
    if bias is None:
        return None
    if isinstance(bias, dict):
        out = np.zeros(vocab, np.float32)
        for k, v in bias.items():
            if not 0 <= int(k) < vocab:
                raise ValueError(f"logit_bias id {k} outside [0, {vocab})")
            out[int(k)] = v
        return out
    if isinstance(bias, torch.Tensor) and bias.is_cuda:
        if bias.dim() != 1 or bias.numel() != vocab:
            raise ValueError(f"logit_bias must be [{vocab}], got {list(bias.shape)}")
        return bias.detach().to(torch.float32).contiguous()
    arr = bias.detach().numpy() if isinstance(bias, torch.Tensor) else np.asarray(bias)
    if arr.shape != (vocab,):
        raise ValueError(f"logit_bias must be [{vocab}], got {list(arr.shape)}")
    return np.ascontiguousarray(arr, dtype=np.float32)


def split_logit_bias(bias, B: int, vocab="V") -> list:
    """One logit bias per row of a batch of B: a 2-D array or tensor [B, vocab] gives row b its row b, anything else -- None, a dict,
    one vector -- is every row's.  ValueError for a 2-D bias of another row count; vocab only words it."""
    if bias is None or isinstance(bias, dict) or getattr(bias, "ndim", 1) != 2:
        return [bias] * B
    if bias.shape[0] != B:
        raise ValueError(f"logit_bias must be [{vocab}] or [{B}, {vocab}], got {list(bias.shape)}")
    return [bias[b] for b in range(B)]


def check_logit_bias(vec, row: int, eos_id: int = -1, min_new_tokens: int = 0, check: bool = True) -> None:
    """The validity rules of include/mgea.h (mgea_row_logits) as ValueErrors naming the row: no NaN, no +inf, at least one finite
    entry, and one besides eos_id when min_new_tokens > 0 bans the EOS.  vec: dense_logit_bias()'s result.  A host vector is always
    checked; a device tensor is read back through ONE reduction, which check=False skips (the caller then guarantees the rules)."""
    if vec is None:
        return
    if isinstance(vec, torch.Tensor):
        if not check:
            return
        fin = torch.isfinite(vec)
        n_fin = fin.sum()
        eos_fin = fin[eos_id].to(n_fin.dtype) if 0 <= eos_id < vec.numel() else torch.zeros_like(n_fin)
        nan, pinf, n_fin, eos_fin = torch.stack([torch.isnan(vec).sum(), (vec == math.inf).sum(), n_fin, eos_fin]).tolist()
    else:
        fin = np.isfinite(vec)
        nan, pinf, n_fin = int(np.isnan(vec).sum()), int((vec == np.inf).sum()), int(fin.sum())
        eos_fin = int(fin[eos_id]) if 0 <= eos_id < vec.size else 0
    if nan:
        raise ValueError(f"row {row}: logit_bias holds NaN")
    if pinf:
        raise ValueError(f"row {row}: logit_bias holds +inf (only finite values and -inf are allowed)")
    if n_fin < 1:
        raise ValueError(f"row {row}: logit_bias bans every token")
    if min_new_tokens > 0 and eos_id >= 0 and n_fin - eos_fin < 1:
        raise ValueError(f"row {row}: logit_bias admits only eos_id {eos_id}, which min_new_tokens {min_new_tokens} bans")


GRAMMAR_MAX_CLASSES, GRAMMAR_MAX_STATES, GRAMMAR_MAX_CELLS = 4096, 4096, 1 << 20
ERR_ID_CLAMPED, ERR_GRAMMAR_BANNED = 1, 2   # bits of the engine's sticky error flags (include/mgea.h, mgea_decoder_error_flags)


@dataclasses.dataclass(eq=False)
class TokenGrammar:
    """A token grammar (include/mgea.h, mgea_decoder_set_grammar): a finite automaton over token classes.  class_of int32 [vocab] is
    the class of every id, next int32 [n_state, n_class] the state after an id of class c in state s, -1 = the class is banned in s.
    The engine masks a row's logits with allowed(state) at every step and moves the state with step(); the methods here are the
    host model of exactly that."""
    class_of: np.ndarray
    next: np.ndarray

    def __post_init__(self):
        self.class_of = np.ascontiguousarray(np.asarray(self.class_of), dtype=np.int32).reshape(-1)
        nx = np.asarray(self.next)
        if nx.ndim != 2:
            raise ValueError(f"TokenGrammar.next must be [n_state, n_class], got {list(nx.shape)}")
        self.next = np.ascontiguousarray(nx, dtype=np.int32)

    @property
    def n_state(self) -> int:
        return int(self.next.shape[0])

    @property
    def n_class(self) -> int:
        return int(self.next.shape[1])

    def check(self, vocab: int) -> None:
        """The rules of mgea_decoder_set_grammar as ValueErrors naming the offender."""
        S, K = self.n_state, self.n_class
        if not 1 <= K <= GRAMMAR_MAX_CLASSES:
            raise ValueError(f"grammar: n_class {K} outside [1, {GRAMMAR_MAX_CLASSES}]")
        if not 1 <= S <= GRAMMAR_MAX_STATES:
            raise ValueError(f"grammar: n_state {S} outside [1, {GRAMMAR_MAX_STATES}]")
        if S * K > GRAMMAR_MAX_CELLS:
            raise ValueError(f"grammar: n_state {S} x n_class {K} exceeds {GRAMMAR_MAX_CELLS} cells")
        if self.class_of.shape != (vocab,):
            raise ValueError(f"grammar: class_of must be [{vocab}], got {list(self.class_of.shape)}")
        bad = np.flatnonzero((self.class_of < 0) | (self.class_of >= K))
        if bad.size:
            raise ValueError(f"grammar: class_of[{int(bad[0])}] = {int(self.class_of[bad[0]])} outside [0, {K})")
        bad = np.argwhere((self.next < -1) | (self.next >= S))
        if bad.size:
            s, c = (int(v) for v in bad[0])
            raise ValueError(f"grammar: next[{s}][{c}] = {int(self.next[s, c])} outside [-1, {S})")
        populated = np.zeros(K, bool)
        populated[self.class_of] = True
        dead = np.flatnonzero(~((self.next >= 0) & populated[None, :]).any(axis=1))
        if dead.size:
            raise ValueError(f"grammar: state {int(dead[0])} admits no class that has an id")

    def allowed(self, state: int) -> np.ndarray:
        """bool [vocab]: the ids the state admits."""
        return self.next[int(state)][self.class_of] >= 0

    def step(self, state: int, id: int) -> int:
        """The state after `id` in `state`; -1 if the state bans it."""
        return int(self.next[int(state), self.class_of[int(id)]])

    def run(self, ids, state: int = 0, strict: bool = True) -> int:
        """The state after the ids.  strict: a banned id raises a ValueError; otherwise it leaves the state alone (what walking a
        prompt needs: its control tokens are not part of the generated language)."""
        state = int(state)
        for t, i in enumerate(ids):
            n = self.step(state, i)
            if n < 0:
                if strict:
                    raise ValueError(f"grammar: id {int(i)} at position {t} is banned in state {state}")
                continue
            state = n
        return state

    def accepts(self, ids, state: int = 0) -> bool:
        """True iff the grammar admits every id in turn, starting from `state`."""
        state = int(state)
        for i in ids:
            state = self.step(state, i)
            if state < 0:
                return False
        return True


KV_PAGE_TOKENS = _lib.KV_PAGE_TOKENS
WINDOW_MAX_RING, WINDOW_MAX_STEPS = 256, 1 << 24


@dataclasses.dataclass(frozen=True)
class KVWindow:
    """The host model of the engine's KV window (include/mgea.h, mgea_decoder_set_window): pure Python, no device.  Every row keeps
    P = sink_pages + ring_pages pages of 64 tokens; logical pages 0 .. S-1, the sink, are never evicted, pages S .. P-1 are a ring.
    At the start of a step a row that is not finished and caches exactly 64 P - 1 tokens evicts its oldest ring page whole.  A row
    has Lp real prompt tokens, and step i (0-based) caches the token it feeds at absolute position Lp + i."""
    sink_pages: int
    ring_pages: int
    max_steps: int

    @property
    def pages(self) -> int:
        return self.sink_pages + self.ring_pages

    @property
    def tokens(self) -> int:
        return self.pages * KV_PAGE_TOKENS

    def check(self, max_ctx: int) -> None:
        """The rules of mgea_decoder_set_window as ValueErrors naming the offending value."""
        S, R = int(self.sink_pages), int(self.ring_pages)
        if S < 1:
            raise ValueError(f"window: sink_pages {S} must be >= 1")
        if R < 2:
            raise ValueError(f"window: ring_pages {R} must be >= 2 (one page would be evicted with the current token in it)")
        if R > WINDOW_MAX_RING:
            raise ValueError(f"window: ring_pages {R} exceeds {WINDOW_MAX_RING}")
        if S + R > int(max_ctx) // KV_PAGE_TOKENS:
            raise ValueError(f"window: sink_pages {S} + ring_pages {R} exceed the {int(max_ctx) // KV_PAGE_TOKENS} whole pages of "
                             f"max_ctx {max_ctx}")
        if not 1 <= int(self.max_steps) <= WINDOW_MAX_STEPS:
            raise ValueError(f"window: max_steps {self.max_steps} outside [1, {WINDOW_MAX_STEPS}]")

    def check_call(self, prompt_width: int, n_steps: int) -> None:
        """What a windowed generation needs: the prompt and its duplicate inside the sink, n_steps <= max_steps."""
        if int(prompt_width) + 1 > self.sink_pages * KV_PAGE_TOKENS:
            raise ValueError(f"prompt width {prompt_width} + 1 exceeds the window's sink of {self.sink_pages} pages "
                             f"({self.sink_pages * KV_PAGE_TOKENS} tokens)")
        if int(n_steps) > int(self.max_steps):
            raise ValueError(f"{n_steps} steps exceed the window's max_steps {self.max_steps}")

    def first_eviction_step(self, prompt_len: int) -> int:
        """i0: the first step that opens with an eviction."""
        return self.tokens - 1 - int(prompt_len)

    def evictions(self, prompt_len: int, step: int) -> int:
        """e(i): the evictions of a row of prompt_len real tokens before step `step` attends (after n steps that all ran:
        evictions(prompt_len, n - 1))."""
        i0 = self.first_eviction_step(prompt_len)
        return 0 if step < i0 else 1 + (int(step) - i0) // KV_PAGE_TOKENS

    def attended(self, prompt_len: int, step: int):
        """The absolute positions step `step` attends, as two ranges: the sink side and the ring side (one of them may be empty
        before the first eviction, when the ranges meet)."""
        e = self.evictions(prompt_len, step)
        last = int(prompt_len) + int(step)
        if e == 0:
            return range(0, last + 1), range(0)
        return range(0, self.sink_pages * KV_PAGE_TOKENS), range((self.sink_pages + e) * KV_PAGE_TOKENS, last + 1)

    def attended_count(self, prompt_len: int, step: int) -> int:
        a, b = self.attended(prompt_len, step)
        return len(a) + len(b)

    def simulate(self, prompt_len: int, n_steps: int, steps=None):
        """The rule, step by step (what the device does, on the host).  Returns (counts, sets): the number of positions every step
        attends, and {step: the set of absolute positions attended} for the steps in `steps` (None: all).  The eviction drops ring
        page S whole."""
        S, P = self.sink_pages, self.pages
        cached = list(range(int(prompt_len)))            # absolute positions in logical order
        counts, sets = [], {}
        for i in range(int(n_steps)):
            if len(cached) == KV_PAGE_TOKENS * P - 1:
                del cached[S * KV_PAGE_TOKENS:(S + 1) * KV_PAGE_TOKENS]
            cached.append(int(prompt_len) + i)
            counts.append(len(cached))
            if steps is None or i in steps:
                sets[i] = set(cached)
        return counts, sets

    @staticmethod
    def evict_rows(page_table, sink_pages: int, ring_pages: int, ctx_len, done, evictions):
        """The evict kernel on host arrays (numpy int32; copies are returned): rows with done == 0 and ctx_len == 64 P - 1 rotate
        page_table[b, S:P] left by one, ctx_len - 64, evictions + 1; the others stay."""
        pt, cl, ev = (np.array(a, dtype=np.int32, copy=True) for a in (page_table, ctx_len, evictions))
        S, P = int(sink_pages), int(sink_pages) + int(ring_pages)
        for b in range(pt.shape[0]):
            if int(np.asarray(done)[b]) == 0 and int(cl[b]) == KV_PAGE_TOKENS * P - 1:
                pt[b, S:P] = np.roll(pt[b, S:P], -1)
                cl[b] -= KV_PAGE_TOKENS
                ev[b] += 1
        return pt, cl, ev


@dataclasses.dataclass
class Truncation:
    """One batch row's truncation rules beyond top-k and top-p (mgea_row_truncation, include/mgea.h), HuggingFace's names and
    semantics.  They apply after temperature, top-k and top-p, in this order, each to the softmax over what the stages before it kept:
    min_p, typical_p (locally typical sampling; it may remove the most likely id), epsilon_cutoff, eta_cutoff.  None or 0 = off;
    typical_p 1 is off too.  A greedy row (top_k 1) ignores them."""
    min_p: Optional[float] = None
    typical_p: Optional[float] = None
    epsilon_cutoff: Optional[float] = None
    eta_cutoff: Optional[float] = None

    def values(self):
        return tuple(0.0 if v is None else float(v) for v in (self.min_p, self.typical_p, self.epsilon_cutoff, self.eta_cutoff))

    @property
    def on(self) -> bool:
        m, t, e, h = self.values()
        return m > 0 or 0 < t < 1 or e > 0 or h > 0

    def check(self, row: int = 0) -> None:
        """ValueError naming the row for what the native call would refuse (MGEA_EINVAL)."""
        m, t, e, h = self.values()
        for name, v, closed in (("min_p", m, True), ("typical_p", t, True), ("epsilon_cutoff", e, False), ("eta_cutoff", h, False)):
            v32 = float(np.float32(v)) if math.isfinite(v) else v
            if not (math.isfinite(v) and 0 <= v32 and (v32 <= 1 if closed else v32 < 1)):
                raise ValueError(f"row {row}: {name} {v} outside [0, 1{']' if closed else ')'}")

    def record(self) -> RowTruncation:
        m, t, e, h = self.values()
        return RowTruncation(min_p=m, typical_p=t, epsilon_cutoff=e, eta_cutoff=h)

    @classmethod
    def of(cls, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> Optional["Truncation"]:
        """The record of the four keyword arguments of the generate surface, or None when all of them are None."""
        if min_p is None and typical_p is None and epsilon_cutoff is None and eta_cutoff is None:
            return None
        return cls(min_p, typical_p, epsilon_cutoff, eta_cutoff)


CLASS_PENALTY_MAX_WINDOW = _lib.CLASS_PENALTY_MAX_WINDOW
CLASS_PENALTY_MAX_VALUE = 1e4


@dataclasses.dataclass
class ClassPenalty:
    """One batch row's windowed penalty over token classes (mgea_row_class_penalty, include/mgea.h): with n_c the number of the row's
    last `window` generated ids (0 = all of them) whose class in the engine's map (DecoderEngine.set_penalty_classes) is c, every id
    of a class with n_c > 0 loses frequency * n_c + presence from its logit, behind the guidance and blend mixes and in front of the
    id-level repetition penalty.  Negative values favour the counted classes.  Both 0 = off: the row is not touched."""
    frequency: float = 0.0
    presence: float = 0.0
    window: int = 0

    @property
    def on(self) -> bool:
        return float(np.float32(self.frequency)) != 0.0 or float(np.float32(self.presence)) != 0.0

    def check(self, row: int = 0, n_steps: Optional[int] = None, n_class: Optional[int] = None) -> None:
        """ValueError naming the row for what the native call would refuse (MGEA_EINVAL): a value that is not finite or beyond
        +-1e4 (as the float32 the record holds), a window outside [0, CLASS_PENALTY_MAX_WINDOW] and, for a row that is on, window 0
        with more than CLASS_PENALTY_MAX_WINDOW steps (n_steps given) and an engine without a class map (n_class given and 0)."""
        for name, v in (("frequency", self.frequency), ("presence", self.presence)):
            v = float(v)
            with np.errstate(over="ignore"):   # (a double beyond float32 is inf as the record's float: refused below)
                v32 = float(np.float32(v))
            if not (math.isfinite(v) and abs(v32) <= CLASS_PENALTY_MAX_VALUE):
                raise ValueError(f"row {row}: {name} {v} must be finite and within +-1e4")
        w = int(self.window)
        if w != self.window or not 0 <= w <= CLASS_PENALTY_MAX_WINDOW:
            raise ValueError(f"row {row}: window {self.window} outside [0, {CLASS_PENALTY_MAX_WINDOW}]")
        if not self.on:
            return
        if w == 0 and n_steps is not None and n_steps > CLASS_PENALTY_MAX_WINDOW:
            raise ValueError(f"row {row}: window 0 (the whole history) with {n_steps} steps: above {CLASS_PENALTY_MAX_WINDOW} steps "
                             "a row that is on needs a window")
        if n_class is not None and n_class <= 0:
            raise ValueError(f"row {row} has a class penalty but no class map is set (set_penalty_classes)")

    def record(self) -> RowClassPenalty:
        return RowClassPenalty(frequency=float(self.frequency), presence=float(self.presence), window=int(self.window), reserved=0)


@dataclasses.dataclass
class RowSampling:
    """One batch row's sampler settings (mgea_row_sampler, include/mgea.h) for DecoderEngine.generate_rows / ops.sample_rows.
    top_k None or 0 = no cut, 1 = greedy (the exact argmax, no temperature division); top_p None = no nucleus cut;
    repetition_penalty None = 1 = none; max_new_tokens 0 = the call's n_steps; stream None = the row's index in the batch (what
    generate() uses).  The row draws its step-t number from Philox counter (stream, t) under key seed.
    logit_bias (None, a dict id -> bias, a host array or a device tensor [vocab]; -inf bans an id) is added to the row's penalized
    logits at every step; min_new_tokens > 0 bans eos_id until the row has produced that many ids (mgea_row_logits).
    grammar_state (None = the row is not constrained): the row's start state in the engine's TokenGrammar (DecoderEngine.set_grammar).
    truncation (None = none): the row's Truncation -- min-p, typical-p, epsilon and eta cutoff behind top-k and top-p.
    class_penalty (None = none): the row's ClassPenalty over the engine's class map (DecoderEngine.set_penalty_classes)."""
    temperature: float = 1.0
    top_k: Optional[int] = 50
    top_p: Optional[float] = None
    repetition_penalty: Optional[float] = None
    eos_id: int = -1
    max_new_tokens: int = 0
    seed: int = 0
    stream: Optional[int] = None
    logit_bias: object = None
    min_new_tokens: int = 0
    # the eleventh constructor argument, after min_new_tokens, and an ordinary attribute afterwards (dataclasses.replace keeps it).  An
    # InitVar rather than a field: dataclasses.fields() stays the ten sampler and logits settings the native records are packed from
    grammar_state: dataclasses.InitVar[Optional[int]] = None
    # the twelfth, carried the same way
    truncation: dataclasses.InitVar[Optional[Truncation]] = None
    # the thirteenth, carried the same way
    class_penalty: dataclasses.InitVar[Optional[ClassPenalty]] = None

    def __post_init__(self, grammar_state, truncation=None, class_penalty=None):
        self.grammar_state = grammar_state
        self.truncation = truncation
        self.class_penalty = class_penalty

    def check(self, row: int, vocab: int, n_steps: Optional[int] = None) -> None:
        """ValueError naming the row for what the native call would refuse (MGEA_EINVAL)."""
        from . import ops
        t = float(self.temperature)
        if not (math.isfinite(t) and t > 0 and math.isfinite(float(np.float32(t))) and float(np.float32(t)) > 0):
            raise ValueError(f"row {row}: temperature must be finite and > 0, got {self.temperature}")
        k = int(self.top_k or 0)
        if not 0 <= k <= vocab:
            raise ValueError(f"row {row}: top_k {k} outside [0, {vocab}]")
        try:
            ops.check_repetition_penalty(self.repetition_penalty)
        except ValueError as e:
            raise ValueError(f"row {row}: {e}") from None
        if n_steps is not None and not 0 <= int(self.max_new_tokens) <= n_steps:
            raise ValueError(f"row {row}: max_new_tokens {self.max_new_tokens} outside [0, {n_steps}]")
        if self.stream is not None and not 0 <= int(self.stream) < 2 ** 32:
            raise ValueError(f"row {row}: stream {self.stream} is not a 32-bit word")
        m = int(self.min_new_tokens)
        if m < 0 or (n_steps is not None and m > n_steps):
            raise ValueError(f"row {row}: min_new_tokens {m} outside [0, {'n_steps' if n_steps is None else n_steps}]")
        if self.truncation is not None:
            if not isinstance(self.truncation, Truncation):
                raise ValueError(f"row {row}: truncation must be a Truncation, got {type(self.truncation).__name__}")
            self.truncation.check(row)
        cp = getattr(self, "class_penalty", None)
        if cp is not None:
            if not isinstance(cp, ClassPenalty):
                raise ValueError(f"row {row}: class_penalty must be a ClassPenalty, got {type(cp).__name__}")
            cp.check(row, n_steps)

    def record(self, row: int) -> RowSampler:
        pen = self.repetition_penalty
        return RowSampler(temperature=float(self.temperature), top_k=int(self.top_k or 0), top_p=float(self.top_p or 0.0),
                          repetition_penalty=1.0 if pen is None else float(pen), eos_id=int(self.eos_id),
                          max_new_tokens=int(self.max_new_tokens), seed=int(self.seed) & (2 ** 64 - 1),
                          stream=(row if self.stream is None else int(self.stream)) & 0xFFFFFFFF, reserved=0)


def pack_rows(rows: Sequence[RowSampling], vocab: int, n_steps: Optional[int] = None):
    """Check every record (ValueError naming the row) and pack them as the C array mgea_row_sampler[B]."""
    rows = list(rows)
    for b, r in enumerate(rows):
        r.check(b, vocab, n_steps)
    return (RowSampler * len(rows))(*[r.record(b) for b, r in enumerate(rows)])


def pack_row_logits(rows: Sequence[RowSampling], vocab: int, device, check: bool = True):
    """The rows' logit_bias / min_new_tokens as the C array mgea_row_logits[B] plus the device tensors it points into (keep them
    alive until the call's stream has passed), or (None, []) when no row sets either -- the caller then makes the unbiased call.
    Every vector is checked (check_logit_bias; check=False skips the read-back of device tensors); rows that share one bias object
    share one upload."""
    rows = list(rows)
    if all(r.logit_bias is None and int(r.min_new_tokens) == 0 for r in rows):
        return None, []
    recs = (RowLogits * len(rows))()
    dense, keep = {}, []
    for b, r in enumerate(rows):
        recs[b].min_new_tokens = int(r.min_new_tokens)
        recs[b].reserved = 0
        if r.logit_bias is None:
            continue
        key = id(r.logit_bias)
        if key not in dense:
            try:
                dense[key] = [dense_logit_bias(r.logit_bias, vocab), None, set()]
            except ValueError as e:
                raise ValueError(f"row {b}: {e}") from None
        vec, dev, seen = dense[key]
        rule = (int(r.eos_id), int(r.min_new_tokens) > 0)
        if rule not in seen:   # the verdict depends on the row only through these
            check_logit_bias(vec, b, int(r.eos_id), int(r.min_new_tokens), check)
            seen.add(rule)
        if dev is None:
            dev = vec.to(device) if isinstance(vec, torch.Tensor) else torch.from_numpy(vec).to(device)
            dense[key][1] = dev
            keep.append(dev)
        recs[b].bias_dev = dev.data_ptr()
    return recs, keep


def pack_truncation(rows: Sequence[RowSampling]):
    """The rows' Truncation records as the C array mgea_row_truncation[B] (rows without one: all off), or None when no row sets one --
    the caller then makes the call without records.  Every record is checked (ValueError naming the row)."""
    rows = list(rows)
    if all(getattr(r, "truncation", None) is None for r in rows):
        return None
    recs = (RowTruncation * len(rows))()
    for b, r in enumerate(rows):
        if r.truncation is not None:
            r.truncation.check(b)
            recs[b] = r.truncation.record()
    return recs


def pack_class_penalty(rows: Sequence[RowSampling], n_steps: Optional[int] = None, n_class: Optional[int] = None):
    """The rows' ClassPenalty records as the C array mgea_row_class_penalty[B] (rows without one: off), or None when no row carries
    one that is on -- the caller then makes the call it always made.  Every record is checked (ValueError naming the row; n_steps
    and n_class as in ClassPenalty.check)."""
    rows = list(rows)
    cps = [getattr(r, "class_penalty", None) for r in rows]
    for b, cp in enumerate(cps):
        if cp is not None:
            cp.check(b, n_steps, n_class)
    if not any(cp is not None and cp.on for cp in cps):
        return None
    recs = (RowClassPenalty * len(rows))()
    for b, cp in enumerate(cps):
        if cp is not None:
            recs[b] = cp.record()
    return recs


@dataclasses.dataclass
class ScoredGeneration:
    """What DecoderEngine.generate_scored returns, all on the device: ids int32 [B, n] (-1 after a row's EOS or budget), logprobs and
    choice_logprobs float32 [B, n] -- the raw and the choice log-probability of every id (include/mgea.h,
    mgea_decoder_generate_rows_scored); 0.0 where ids is -1."""
    ids: torch.Tensor
    logprobs: torch.Tensor
    choice_logprobs: torch.Tensor

    def first_rows(self, n: int, scored: bool = True):
        """Rows [0, n) -- the callers' rows of a batch with shadow rows behind them; scored=False: their ids alone."""
        if not scored:
            return self.ids[:n]
        return ScoredGeneration(self.ids[:n], self.logprobs[:n], self.choice_logprobs[:n])


def pack_force_ids(force_ids, B: int, n_steps: int, vocab: int):
    """Forced ids as an int32 [B, n_steps] matrix, -1 = the step is free.  force_ids: None (-> None), B id lists (ragged allowed,
    padded with -1; None or [] = a free row) or an int tensor [B, <= n_steps].  Host data outside [-1, vocab) raises a ValueError
    naming the row; a DEVICE tensor is not read back (the kernel clamps ids >= vocab and sets the engine's error flag)."""
    if force_ids is None:
        return None
    if isinstance(force_ids, torch.Tensor):
        if force_ids.dim() != 2 or force_ids.shape[0] != B or force_ids.shape[1] > n_steps or force_ids.is_floating_point():
            raise ValueError(f"force_ids must be an int tensor [{B}, <= {n_steps}], got {list(force_ids.shape)} {force_ids.dtype}")
        t = force_ids.to(torch.int32)
        if not t.is_cuda:
            bad = ((t < -1) | (t >= vocab)).any(dim=1).nonzero()
            if bad.numel():
                b = int(bad[0])
                raise ValueError(f"row {b}: force_ids outside [-1, {vocab})")
        if t.shape[1] < n_steps:
            t = torch.cat([t, torch.full((B, n_steps - t.shape[1]), -1, dtype=torch.int32, device=t.device)], dim=1)
        return t.contiguous()
    rows = list(force_ids)
    if len(rows) != B:
        raise ValueError(f"{B} prompts but {len(rows)} force_ids rows")
    out = np.full((B, n_steps), -1, np.int32)
    for b, r in enumerate(rows):
        r = np.asarray([] if r is None else list(r), dtype=np.int64).reshape(-1)
        if r.size > n_steps:
            raise ValueError(f"row {b}: {r.size} forced ids for {n_steps} steps")
        if r.size and (r.min() < -1 or r.max() >= vocab):
            raise ValueError(f"row {b}: force_ids outside [-1, {vocab})")
        out[b, :r.size] = r
    return torch.from_numpy(out)


def check_guidance(shadow_rows, scales, B: int) -> None:
    """The pair rules of mgea_decoder_generate_rows_guided (include/mgea.h, mgea_row_guidance) as ValueErrors naming the row:
    shadow_row in [-1, B) and not the row itself, a shadow row is not conditional itself, no row is the shadow of two rows, a
    conditional row's scale is finite and >= 0.  Pure host code."""
    shadow_rows = [int(u) for u in shadow_rows]
    if len(shadow_rows) != B or len(scales) != B:
        raise ValueError(f"guidance: {len(shadow_rows)} shadow rows and {len(scales)} scales for {B} rows")
    for b, u in enumerate(shadow_rows):
        if not -1 <= u < B:
            raise ValueError(f"row {b}: shadow_row {u} outside [-1, {B})")
        if u == b:
            raise ValueError(f"row {b}: a row cannot be its own shadow")
        if u < 0:
            continue
        s = float(scales[b])
        if not (math.isfinite(s) and 0 <= s <= float(np.finfo(np.float32).max)):   # (finite as the float32 the record holds)
            raise ValueError(f"row {b}: guidance scale {scales[b]} must be finite and >= 0")
    owner = {}
    for b, u in enumerate(shadow_rows):
        if u < 0:
            continue
        if shadow_rows[u] >= 0:
            raise ValueError(f"row {b}: its shadow row {u} is conditional itself (shadow_row {shadow_rows[u]})")
        if u in owner:
            raise ValueError(f"row {b}: row {u} is already the shadow of row {owner[u]}")
        owner[u] = b


def pack_guided(prompts, negative_prompts, rows, guidance_scale, max_batch: int, force_ids=None):
    """The host half of DecoderEngine.generate_guided (no device): n prompts, of which those with a negative prompt are conditional,
    become one batch -- the callers' rows 0 .. n-1, then one shadow row per pair in the order of their conditional rows, each with its
    negative prompt and its conditional row's RowSampling (the engine samples a shadow row with its conditional row's record anyway).
    negative_prompts[i] None = row i is not guided; guidance_scale: one value, or one per prompt (read only for the guided ones).
    force_ids (None, or n id lists as in pack_force_ids; an int tensor [n, steps] gets free rows behind it): the shadow rows take
    their conditional rows' ids inside the engine.  Returns (prompts, rows, shadow_rows, scales, force_ids) of the whole batch.
    ValueError naming the row: a bad scale, an empty negative prompt, a shadow row that would not fit into max_batch."""
    prompts = prompts.tolist() if isinstance(prompts, torch.Tensor) else [list(p) for p in prompts]
    rows = list(rows)
    n = len(prompts)
    negative_prompts = [None] * n if negative_prompts is None else list(negative_prompts)
    if len(rows) != n:
        raise ValueError(f"{n} prompts but {len(rows)} sampler rows")
    if len(negative_prompts) != n:
        raise ValueError(f"{n} prompts but {len(negative_prompts)} negative prompts")
    if isinstance(guidance_scale, (list, tuple, np.ndarray, torch.Tensor)):
        per = [float(v) for v in guidance_scale]
        if len(per) != n:
            raise ValueError(f"guidance_scale: {len(per)} values for {n} prompts")
    else:
        per = [float(guidance_scale)] * n
    all_prompts, all_rows = list(prompts), list(rows)
    shadow, scales = [-1] * n, [0.0] * n
    for i, neg in enumerate(negative_prompts):
        if neg is None:
            continue
        neg = neg.tolist() if isinstance(neg, torch.Tensor) else list(neg)
        if len(neg) < 1:
            raise ValueError(f"row {i}: empty negative prompt")
        if not (math.isfinite(per[i]) and per[i] >= 0):
            raise ValueError(f"row {i}: guidance scale {per[i]} must be finite and >= 0")
        u = len(all_prompts)
        if u >= int(max_batch):
            n_pairs = sum(p is not None for p in negative_prompts)
            raise ValueError(f"row {i}: its shadow row {u} does not fit: {n} prompts + {n_pairs} negative prompts exceed max_batch {max_batch}")
        shadow[i], scales[i] = u, per[i]
        all_prompts.append(neg)
        all_rows.append(rows[i])
        shadow.append(-1)
        scales.append(0.0)
    extra = len(all_prompts) - n
    if isinstance(force_ids, torch.Tensor):
        if force_ids.dim() == 2 and extra:
            pad = torch.full((extra, force_ids.shape[1]), -1, dtype=force_ids.dtype, device=force_ids.device)
            force_ids = torch.cat([force_ids, pad], dim=0)
    elif force_ids is not None:
        force_ids = list(force_ids)
        if len(force_ids) != n:
            raise ValueError(f"{n} prompts but {len(force_ids)} force_ids rows")
        force_ids = force_ids + [None] * extra
    check_guidance(shadow, scales, len(all_prompts))
    return all_prompts, all_rows, shadow, scales, force_ids


BLEND_MAX_ROWS = _lib.BLEND_MAX_ROWS


def check_blend(leader, weights, B: int, shadow_rows=None) -> None:
    """The group rules of mgea_decoder_generate_rows_blended (include/mgea.h, mgea_row_blend) as ValueErrors naming the row: leader in
    [-1, B), a named leader names itself, a group has 2 to BLEND_MAX_ROWS rows, a grouped row's weight is finite (as the float32 the
    record holds), a group's weights sum to 1 within 1e-3, and -- with the batch's shadow_rows (check_guidance) -- a grouped row is
    neither the conditional nor the shadow row of a guidance pair.  Pure host code."""
    leader = [int(l) for l in leader]
    if len(leader) != B or len(weights) != B:
        raise ValueError(f"blend: {len(leader)} leaders and {len(weights)} weights for {B} rows")
    f32_max = float(np.finfo(np.float32).max)
    for b, l in enumerate(leader):
        if not -1 <= l < B:
            raise ValueError(f"row {b}: leader {l} outside [-1, {B})")
        if l < 0:
            continue
        if leader[l] != l:
            raise ValueError(f"row {b}: its leader row {l} does not name itself (leader {leader[l]})")
        w = float(weights[b])
        if not (math.isfinite(w) and abs(w) <= f32_max):
            raise ValueError(f"row {b}: weight {weights[b]} must be finite")
    paired = set()
    for b, u in enumerate([] if shadow_rows is None else [int(u) for u in shadow_rows]):
        if u >= 0:
            paired.update((b, u))
    size, total = {}, {}
    for b, l in enumerate(leader):
        if l < 0:
            continue
        if b in paired:
            raise ValueError(f"row {b} is in a blend group and in a guidance pair")
        size[l] = size.get(l, 0) + 1
        if size[l] > BLEND_MAX_ROWS:
            raise ValueError(f"row {b}: the group of leader row {l} has more than {BLEND_MAX_ROWS} rows")
        total[l] = total.get(l, 0.0) + float(np.float32(weights[b]))
    for l in sorted(size):
        if size[l] < 2:
            raise ValueError(f"row {l}: a group of {size[l]} row (a group has 2 to {BLEND_MAX_ROWS})")
        if not abs(total[l] - 1.0) <= 1e-3:
            raise ValueError(f"row {l}: the weights of its group sum to {total[l]:g}, not 1 (a blend is an affine combination)")


def pack_blended(prompt_groups, weights, rows, max_batch: int, force_ids=None):
    """The host half of DecoderEngine.generate_blended (no device): n groups of 1 to BLEND_MAX_ROWS prompts become one batch -- group
    i's first prompt, its leader, at row i, then the other members of every group in the order of their leaders, each with its
    leader's RowSampling (the engine samples a member with its leader's record anyway).  weights[i]: one value per prompt of group i;
    a group of one prompt is a plain row (its weight is not read).  force_ids (None, n id lists as in pack_force_ids, or an int tensor
    [n, steps]): a member gets its leader's ids.  Returns (prompts, rows, leader, weight, force_ids) of the whole batch.
    ValueError naming the group or the row: an empty group or prompt, more than BLEND_MAX_ROWS prompts, a weight count that differs
    from the group's, a member that would not fit into max_batch, and what check_blend refuses."""
    groups = []
    for g in prompt_groups:
        g = g.tolist() if isinstance(g, torch.Tensor) else list(g)
        groups.append([list(p.tolist() if isinstance(p, torch.Tensor) else p) for p in g]
                      if g and isinstance(g[0], (list, tuple, torch.Tensor)) else [list(g)])
    rows = list(rows)
    n = len(groups)
    weights = list(weights)
    if len(rows) != n or len(weights) != n:
        raise ValueError(f"{n} prompt groups but {len(rows)} sampler rows and {len(weights)} weight lists")
    if n > int(max_batch):
        raise ValueError(f"{n} prompt groups exceed max_batch {max_batch}")
    total = sum(len(g) for g in groups)
    all_prompts, all_rows = [None] * n, list(rows)
    leader, weight, src = [-1] * n, [0.0] * n, list(range(n))
    for i, g in enumerate(groups):
        w = [float(v) for v in (weights[i].tolist() if hasattr(weights[i], "tolist") else weights[i])]
        if not 1 <= len(g) <= BLEND_MAX_ROWS:
            raise ValueError(f"group {i}: {len(g)} prompts outside [1, {BLEND_MAX_ROWS}]")
        if any(len(p) < 1 for p in g):
            raise ValueError(f"group {i}: empty prompt")
        if len(w) != len(g):
            raise ValueError(f"group {i}: {len(w)} weights for {len(g)} prompts")
        all_prompts[i] = g[0]
        if len(g) == 1:
            continue
        leader[i], weight[i] = i, w[0]
        for p, wk in zip(g[1:], w[1:]):
            u = len(all_prompts)
            if u >= int(max_batch):
                raise ValueError(f"group {i}: its member row {u} does not fit: {total} prompts in {n} groups exceed max_batch {max_batch}")
            all_prompts.append(p)
            all_rows.append(rows[i])
            leader.append(i)
            weight.append(wk)
            src.append(i)
    if isinstance(force_ids, torch.Tensor):
        if force_ids.dim() == 2 and len(src) > n:
            force_ids = force_ids[torch.tensor(src, device=force_ids.device)]
    elif force_ids is not None:
        force_ids = list(force_ids)
        if len(force_ids) != n:
            raise ValueError(f"{n} prompt groups but {len(force_ids)} force_ids rows")
        force_ids = [force_ids[i] for i in src]
    check_blend(leader, weight, len(all_prompts))
    return all_prompts, all_rows, leader, weight, force_ids


SCHEDULE_MAX_SEGMENTS = 8


@dataclasses.dataclass(frozen=True)
class RowSchedule:
    """One batch row's prompt schedule (mgea_row_schedule, include/mgea.h) and the host model of its rule: the row has
    len(thresholds) + 1 prompt variants and, at the start of every decode step, is in segment #{s : thresholds[s] <= k}, where k is
    its step index (key 0) or its grammar state (key 1).  RowSchedule() is a plain row: one segment, never switched."""
    thresholds: Sequence[int] = ()
    key: int = 0

    @property
    def n_segments(self) -> int:
        return len(self.thresholds) + 1

    def check(self, row: int = 0) -> None:
        """ValueError naming the row for what the native call would refuse by the record alone."""
        if not 1 <= self.n_segments <= SCHEDULE_MAX_SEGMENTS:
            raise ValueError(f"row {row}: n_segments {self.n_segments} outside [1, {SCHEDULE_MAX_SEGMENTS}]")
        if self.key not in (0, 1):
            raise ValueError(f"row {row}: key {self.key} (0 = step index, 1 = grammar state)")
        th = [int(t) for t in self.thresholds]
        for s, t in enumerate(th):
            if not 0 <= t < 2 ** 31:
                raise ValueError(f"row {row}: threshold[{s}] = {t} outside [0, 2^31)")
            if s and t < th[s - 1]:
                raise ValueError(f"row {row}: thresholds not ascending ({t} after {th[s - 1]})")

    def record(self) -> "_lib.RowSchedule":
        rec = _lib.RowSchedule(n_segments=self.n_segments, key=int(self.key), reserved=0)
        for s, t in enumerate(self.thresholds):
            rec.threshold[s] = int(t)
        return rec

    def segment_at(self, key: int) -> int:
        """The segment a row that is not finished is in at the start of a step whose key value is `key`."""
        seg = 0
        for t in self.thresholds:
            seg += 1 if int(t) <= int(key) else 0
        return seg


def pack_scheduled(prompt_segments, schedules, rows, max_batch: int):
    """The host half of DecoderEngine.generate_scheduled (no device): per row its prompt variants (a list of id lists, all of one
    length; a bare id list = one variant) and its RowSchedule (None = plain).  Returns (variants, schedules, n_seg_max): variants[s] =
    the B prompts of segment s, a row with fewer segments repeating its last one.  ValueError naming the row: a variant count that
    differs from the schedule's n_segments, variants of different lengths, a prompt wider than a page, key 1 without grammar_state."""
    rows = list(rows)
    segs = []
    for p in prompt_segments:
        p = p.tolist() if isinstance(p, torch.Tensor) else list(p)
        segs.append([list(v) for v in p] if p and isinstance(p[0], (list, tuple)) else [list(p)])
    n = len(segs)
    schedules = [RowSchedule() if s is None else s for s in ([None] * n if schedules is None else list(schedules))]
    if len(schedules) != n or len(rows) != n:
        raise ValueError(f"{n} prompts but {len(schedules)} schedules and {len(rows)} sampler rows")
    if n > int(max_batch):
        raise ValueError(f"{n} prompts exceed max_batch {max_batch}")
    for b, (vs, sc) in enumerate(zip(segs, schedules)):
        sc.check(b)
        if len(vs) != sc.n_segments:
            raise ValueError(f"row {b}: {len(vs)} prompt variants for a schedule of {sc.n_segments} segments")
        if len(vs[0]) < 1:
            raise ValueError(f"row {b}: empty prompt")
        if any(len(v) != len(vs[0]) for v in vs):
            raise ValueError(f"row {b}: prompt variants of different lengths {[len(v) for v in vs]}")
        if sc.n_segments > 1 and len(vs[0]) > KV_PAGE_TOKENS:
            raise ValueError(f"row {b}: a scheduled prompt of {len(vs[0])} tokens exceeds one page of {KV_PAGE_TOKENS}")
        if sc.n_segments > 1 and sc.key == 1 and rows[b].grammar_state is None:
            raise ValueError(f"row {b}: key 1 (grammar state) on a row without a grammar_state")
    n_seg_max = max(sc.n_segments for sc in schedules)
    variants = [[vs[min(s, len(vs) - 1)] for vs in segs] for s in range(n_seg_max)]
    return variants, schedules, n_seg_max
