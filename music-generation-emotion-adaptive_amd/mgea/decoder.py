"""Host side of the MI355X decoder engine: weight arena, handle lifetime, torch tensor plumbing.

PyTorch is used only for device memory, streams and (in mgea.dist) the RCCL broadcast; all
arithmetic happens in libmgea_hip.so.  Mirrors GPTWithKV / sample_kvcache of the reference
(api_cache.py:76-106, 159-184) -- see generate_music/generate.py for the drop-in names.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import DecoderConfig, RowClassPenalty, RowLogits, RowSampler, RowTruncation, SamplerConfig, check, ptr

_LAYER_TENSORS = ["ln1.weight", "ln1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                  "attn.out_proj.bias", "ln2.weight", "ln2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
                  "mlp.2.bias"]


def remap_state_dict(old_sd: Dict) -> Dict:
    """Training-checkpoint names -> model names, same mapping as the reference's
    remap_state_dict (api_cache.py:118-134): emb->tok_emb, pos->pos_emb, fc->head,
    tr.layers.N.{self_attn,norm1,norm2,linear1,linear2} -> layers.N.{attn,ln1,ln2,mlp.0,mlp.2}."""
    table = [(r"^emb\.weight$", "tok_emb.weight"), (r"^pos$", "pos_emb"), (r"^fc\.", "head."),
             (r"^tr\.layers\.(\d+)\.self_attn", r"layers.\1.attn"), (r"^tr\.layers\.(\d+)\.norm1", r"layers.\1.ln1"),
             (r"^tr\.layers\.(\d+)\.norm2", r"layers.\1.ln2"), (r"^tr\.layers\.(\d+)\.linear1", r"layers.\1.mlp.0"),
             (r"^tr\.layers\.(\d+)\.linear2", r"layers.\1.mlp.2")]
    new_sd = {}
    for k, v in old_sd.items():
        k2 = k
        for pat, rep in table:
            k2 = re.sub(pat, rep, k2)
        new_sd[k2] = v
    return new_sd


def geometry_from_state_dict(sd: Dict) -> Dict[str, int]:
    """Infer (n_layer, seq_len, d_model, vocab, d_ff) from tensor shapes like api_cache.py:31-37."""
    sd = remap_state_dict(sd)
    n_layer = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))
    seq_len, d_model = (int(x) for x in sd["pos_emb"].shape)
    return dict(n_layer=n_layer, seq_len=seq_len, d_model=d_model, vocab=int(sd["tok_emb.weight"].shape[0]),
                d_ff=int(sd["layers.0.mlp.0.weight"].shape[0]))


def _as_f32(t, device):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def arena_layout(geometry: Dict[str, int], n_head: int = 8):
    """(offsets, total_floats) of the canonical weight arena for a geometry -- what a rank that
    only RECEIVES the RCCL broadcast needs to size its buffer."""
    lib = _lib.load()
    cfg = DecoderConfig(vocab=geometry["vocab"], seq_len=geometry["seq_len"], d_model=geometry["d_model"],
                        n_head=n_head, n_layer=geometry["n_layer"], d_ff=geometry["d_ff"], max_batch=1, max_ctx=1,
                        dtype=_lib.DTYPE_F32, block_mode=0, pos_mode=0, ln_eps=1e-5)
    n, total = C.c_int32(0), C.c_int64(0)
    check(lib.mgea_decoder_arena_layout(C.byref(cfg), None, C.byref(n), C.byref(total)))
    offs = (C.c_int64 * n.value)()
    check(lib.mgea_decoder_arena_layout(C.byref(cfg), offs, C.byref(n), C.byref(total)))
    return list(offs), total.value


# training-checkpoint tensor-name suffixes of the matrices the fp16 mode stores in fp16 (everything else stays fp32)
F16_ROUNDED_KEYS = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight", "fc.weight",
                    "attn.in_proj_weight", "attn.out_proj.weight", "mlp.0.weight", "mlp.2.weight", "head.weight")


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


def _prompt_ids(prompts):
    """prompts (id lists, ragged ok, or an int tensor [B, Tp]) -> (int32 ids [B, Tp] on the host, lens [B] or None)"""
    if isinstance(prompts, torch.Tensor):
        return prompts.to(torch.int32), None
    B = len(prompts)
    if B == 0 or min(len(p) for p in prompts) < 1:
        raise ValueError("empty prompt")
    Tp = max(len(p) for p in prompts)
    ids = torch.zeros(B, Tp, dtype=torch.int32)
    for b, p in enumerate(prompts):
        ids[b, :len(p)] = torch.tensor(list(p), dtype=torch.int32)
    lens = None if all(len(p) == Tp for p in prompts) else torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    return ids, lens


class DecoderEngine:
    """One native decoder handle on one GPU."""

    # pos_mode "causal" (MGEA_POS_CAUSAL in include/mgea.h): a standard causal GPT -- true positions, a causal mask in every prefill,
    # every token fed once; "reference": the reference's unmasked model with position row 0 on every step
    POS_MODES = {"reference": _lib.POS_REFERENCE, "absolute": _lib.POS_ABSOLUTE, "causal": _lib.POS_CAUSAL}
    SCORE_PREFILL_LOGITS_BYTES = 256 << 20   # score_prefill: the cap of one chunk's logits buffer

    def __init__(self, state_dict: Optional[Dict], n_head: int = 8, max_batch: int = 64, max_ctx: Optional[int] = None,
                 device="cuda:0", block_mode: str = "kv", pos_mode: str = "reference", geometry: Optional[Dict] = None,
                 arena: Optional[torch.Tensor] = None, ln_eps: float = 1e-5, dtype: str = "f32"):
        """dtype "f32": the parity mode (fp32 storage, exact-fp32 MFMA; bit-exact greedy ids against the reference).
        dtype "f16": the perf mode of BASELINE configs[4] -- the five projection-matrix kinds and the KV pages are stored
        in fp16 (half the bytes a decode step streams), accumulation / residual stream / LayerNorm / softmax / logits
        stay fp32.  The model it serves is exactly the reference with those matrices rounded to fp16 (F16_ROUNDED_KEYS);
        what differs from an fp32 run of THAT model is only activation and KV rounding (tests/test_gpu_f16.py)."""
        if dtype not in ("f32", "f16"):
            raise ValueError("decoder dtype must be 'f32' or 'f16'")
        if pos_mode not in self.POS_MODES:
            raise ValueError("decoder pos_mode must be 'reference', 'absolute' or 'causal'")
        self.dtype = dtype
        self.causal = pos_mode == "causal"
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DecoderEngine needs a ROCm device ('cuda:N'); there is no CPU path")
        geo = dict(geometry) if geometry is not None else geometry_from_state_dict(state_dict)
        self.vocab, self.seq_len, self.d_model = geo["vocab"], geo["seq_len"], geo["d_model"]
        self.n_layer, self.d_ff, self.n_head = geo["n_layer"], geo["d_ff"], int(n_head)
        self.max_batch = int(max_batch)
        self.max_ctx = int(max_ctx if max_ctx is not None else self.seq_len)
        self.cfg = DecoderConfig(vocab=self.vocab, seq_len=self.seq_len, d_model=self.d_model, n_head=self.n_head,
                                 n_layer=self.n_layer, d_ff=self.d_ff, max_batch=self.max_batch, max_ctx=self.max_ctx,
                                 dtype=_lib.DTYPE_F16 if dtype == "f16" else _lib.DTYPE_F32,
                                 block_mode=_lib.BLOCK_PRELN_GELU if block_mode == "kv" else _lib.BLOCK_POSTLN_RELU,
                                 pos_mode=self.POS_MODES[pos_mode],
                                 ln_eps=ln_eps)
        n = C.c_int32(0)
        total = C.c_int64(0)
        check(self.lib.mgea_decoder_arena_layout(C.byref(self.cfg), None, C.byref(n), C.byref(total)))
        offs = (C.c_int64 * n.value)()
        check(self.lib.mgea_decoder_arena_layout(C.byref(self.cfg), offs, C.byref(n), C.byref(total)))
        self.offsets = list(offs)
        self.arena_floats = total.value
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        if arena is not None:
            if arena.numel() != self.arena_floats or arena.dtype != torch.float32 or arena.device != self.device:
                raise ValueError("arena tensor has the wrong size / dtype / device")
            self.arena = arena
        else:
            self.arena = self.pack_arena(state_dict, self.cfg_dict(), self.offsets, self.arena_floats, self.device)
        torch.cuda.synchronize(self.device)
        h = C.c_void_p(0)
        check(self.lib.mgea_decoder_create(C.byref(self.cfg), ptr(self.arena), C.byref(h)))
        self.h = h
        self.grammar: Optional[TokenGrammar] = None
        self._cpen_n_class = 0   # the n_class of the penalty class map (set_penalty_classes); 0: none is set
        self.window: Optional[KVWindow] = None
        self._cur_batch = 0
        self._epoch = 0  # bumps whenever the native cache is reset (guards stale `presents`)
        self._len = 0

    def cfg_dict(self):
        return dict(vocab=self.vocab, seq_len=self.seq_len, d_model=self.d_model, n_layer=self.n_layer, d_ff=self.d_ff)

    @staticmethod
    def tensor_names(n_layer: int) -> List[str]:
        names = ["tok_emb.weight", "pos_emb"]
        for i in range(n_layer):
            names += [f"layers.{i}.{t}" for t in _LAYER_TENSORS]
        return names + ["head.weight", "head.bias"]

    @staticmethod
    def pack_arena(state_dict, geo, offsets, total, device) -> torch.Tensor:
        """Copy every tensor into its slot of the single fp32 arena (canonical order of mgea.h)."""
        sd = remap_state_dict(state_dict)
        names = DecoderEngine.tensor_names(geo["n_layer"])
        missing = [k for k in names if k not in sd]
        if missing:
            raise KeyError(f"Missing key(s) in state_dict: {missing[:4]}{'...' if len(missing) > 4 else ''}")
        arena = torch.zeros(total, dtype=torch.float32, device=device)
        for name, off in zip(names, offsets):
            t = _as_f32(sd[name], device).reshape(-1)
            arena[off:off + t.numel()].copy_(t)
        return arena

    # ------------------------------------------------------------------ lifetime
    def refresh_weights(self):
        """Call after rewriting `self.arena` in place: the engine keeps a decode-layout copy of the matrices."""
        with self._on_stream():
            check(self.lib.mgea_decoder_refresh_weights(self.h, self._sp()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mgea_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    @contextlib.contextmanager
    def _on_stream(self):
        """Run on the engine's own stream (hipGraph capture is illegal on the null stream),
        ordered after / before the caller's current stream."""
        outer = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(outer)
        with torch.cuda.stream(self.stream):
            yield
        outer.wait_stream(self.stream)

    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _check_ids(self, ids: torch.Tensor) -> bool:
        """Token ids outside the vocabulary: nn.Embedding raises IndexError in the reference (api_cache.py:99).
        A HOST tensor is checked here, before the upload, at no GPU cost.  A DEVICE tensor is not read back (that
        would put a host sync in front of every call of the reference's own loop, api_cache.py:166-168): the
        kernels clamp such ids and set a sticky device flag, see id_errors().  Returns True if it checked."""
        if ids.is_cuda:
            return False
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.vocab):
            raise IndexError("index out of range in self")  # what nn.Embedding raises on CPU
        return True

    def id_errors(self, raise_error: bool = True) -> int:
        """Read and clear the engine's sticky device flags (ONE stream sync): bit 0 (ERR_ID_CLAMPED) = some token id handed over as a
        device tensor since the last call was outside the vocabulary (and was clamped) -- the IndexError; bit 1 (ERR_GRAMMAR_BANNED) =
        a forced id was banned by its row's grammar state (the state stayed where it was) -- reported in the return value only."""
        flags = C.c_int32(0)
        with self._on_stream():
            check(self.lib.mgea_decoder_error_flags(self.h, C.byref(flags), self._sp()))
        if raise_error and (flags.value & 1):
            raise IndexError("index out of range in self")
        return flags.value

    @staticmethod
    def sampler(temperature=1.0, top_k: Optional[int] = 50, top_p: Optional[float] = None, eos_id: int = -1,
                seed: int = 0) -> SamplerConfig:
        return SamplerConfig(temperature=float(temperature), top_k=int(top_k) if top_k else 0,
                             top_p=float(top_p) if top_p else 0.0, eos_id=int(eos_id), seed=int(seed) & (2 ** 64 - 1))

    # ------------------------------------------------------------------ token grammar
    def set_grammar(self, grammar: Optional[TokenGrammar]) -> None:
        """Upload a TokenGrammar (checked here: ValueError naming the offender), or None to clear it.  One grammar per engine, shared
        by the rows; a row takes part through RowSampling.grammar_state.  An upload of the same shape keeps the captured graphs."""
        if grammar is None:
            with self._on_stream():
                check(self.lib.mgea_decoder_set_grammar(self.h, None, None, 0, 0, self._sp()))
            self.grammar = None
            return
        grammar.check(self.vocab)
        with self._on_stream():
            check(self.lib.mgea_decoder_set_grammar(self.h, grammar.class_of.ctypes.data_as(C.c_void_p), grammar.next.ctypes.data_as(C.c_void_p),
                                                    grammar.n_state, grammar.n_class, self._sp()))
        self.grammar = grammar

    def grammar_states(self) -> torch.Tensor:
        """int32 [B] on the device: every row's state after the last grammar generation (-1: the row had none)."""
        with self._on_stream():
            out = torch.empty(self._cur_batch, dtype=torch.int32, device=self.device)
            check(self.lib.mgea_decoder_grammar_states(self.h, ptr(out), self._sp()))
        return out

    def grammar_info(self):
        out = (C.c_int64 * 4)()
        check(self.lib.mgea_decoder_grammar_info(self.h, out))
        return dict(n_state=out[0], n_class=out[1], uploads=out[2], grammar_steps=out[3])

    # ------------------------------------------------------------------ penalty classes
    def set_penalty_classes(self, class_of) -> None:
        """Set the map from ids to penalty classes (mgea_decoder_set_penalty_classes), or None to clear it.  class_of: vocab ints in
        [-1, n_class), n_class = the largest class + 1; -1 = the id is in no class, never counted and never penalised.  One map per
        engine, shared by the rows; a row takes part through RowSampling.class_penalty.  ValueError naming the offending id."""
        if class_of is None:
            with self._on_stream():
                check(self.lib.mgea_decoder_set_penalty_classes(self.h, None, 0, self._sp()))
            self._cpen_n_class = 0
            return
        m = np.ascontiguousarray(np.asarray(class_of.cpu() if isinstance(class_of, torch.Tensor) else class_of), dtype=np.int64)
        if m.ndim != 1 or m.shape[0] != self.vocab:
            raise ValueError(f"class_of must hold one class per id: {self.vocab} values, got shape {tuple(m.shape)}")
        if m.shape[0] > 14336:
            raise ValueError(f"penalty classes need a vocabulary of at most 14336 ids, got {m.shape[0]}")
        n_class = int(m.max()) + 1
        bad = np.nonzero(m < -1)[0]
        if bad.size:
            raise ValueError(f"class_of[{int(bad[0])}] = {int(m[bad[0]])} is below -1")
        if n_class < 1:
            raise ValueError("class_of puts no id into a class")
        m32 = m.astype(np.int32)
        with self._on_stream():
            check(self.lib.mgea_decoder_set_penalty_classes(self.h, m32.ctypes.data_as(C.c_void_p), n_class, self._sp()))
        self._cpen_n_class = n_class

    def class_penalty_info(self):
        """The n_class of the map that is set (0 = none), and the rows that were on and the class-penalised decode steps of the last
        generation (both 0 if it was not class-penalised)."""
        out = (C.c_int64 * 3)()
        check(self.lib.mgea_decoder_class_penalty_info(self.h, out))
        return dict(n_class=int(out[0]), rows=int(out[1]), class_penalized_steps=int(out[2]))

    # ------------------------------------------------------------------ KV window
    def set_window(self, sink_pages: int = 1, ring_pages: Optional[int] = None, max_steps: Optional[int] = None) -> None:
        """Set the engine's KV window (KVWindow; include/mgea.h, mgea_decoder_set_window): generate*, generate_rows, generate_scored
        and score then accept n_steps up to max_steps whatever max_ctx is -- the prompt (width + 1 <= 64 * sink_pages) stays pinned
        in the sink while the oldest generated tokens leave the ring a page at a time.  ring_pages None = all the remaining pages of
        max_ctx; max_steps None = 16 * max_ctx (the histories cost max_batch * max_steps * 16 bytes).  sink_pages 0 clears the
        window: the engine then behaves exactly as one that never had it.  ValueError naming the offending value."""
        if int(sink_pages) == 0:
            with self._on_stream():
                check(self.lib.mgea_decoder_set_window(self.h, 0, 0, 0, self._sp()))
            self.window = None
            return
        if ring_pages is None:
            ring_pages = min(self.max_ctx // KV_PAGE_TOKENS - int(sink_pages), WINDOW_MAX_RING)
        w = KVWindow(int(sink_pages), int(ring_pages), int(16 * self.max_ctx if max_steps is None else max_steps))
        w.check(self.max_ctx)
        if self.cfg.block_mode != _lib.BLOCK_PRELN_GELU or self.cfg.pos_mode != _lib.POS_REFERENCE:   # (causal engines too)
            raise ValueError("window: needs the KV-cache block mode and the reference's position mode")
        with self._on_stream():
            check(self.lib.mgea_decoder_set_window(self.h, w.sink_pages, w.ring_pages, w.max_steps, self._sp()))
        self.window = w

    def window_info(self) -> Optional[KVWindow]:
        """The window the native engine holds now (None: none)."""
        out = (C.c_int32 * 3)()
        check(self.lib.mgea_decoder_window_info(self.h, out, None, self._sp()))
        return KVWindow(out[0], out[1], out[2]) if out[0] > 0 else None

    def window_evictions(self) -> List[int]:
        """The rows' eviction counts of the last generation (one stream sync); KVWindow.evictions is their closed form."""
        out = (C.c_int32 * 3)()
        ev = (C.c_int32 * max(self._cur_batch, 1))()
        with self._on_stream():
            check(self.lib.mgea_decoder_window_info(self.h, out, ev, self._sp()))
        return list(ev)[:self._cur_batch]

    def _start_states(self, rows):
        """The rows' grammar start states as a C int32 [B] array, or None when no row has one (the caller then makes the call it
        always made).  ValueError naming the row for what mgea_decoder_generate_rows_grammar would refuse."""
        if all(r.grammar_state is None for r in rows):
            return None
        g = getattr(self, "grammar", None)
        out = (C.c_int32 * len(rows))()
        for b, r in enumerate(rows):
            st = -1 if r.grammar_state is None else int(r.grammar_state)
            if st != -1 and g is None:
                raise ValueError(f"row {b}: grammar_state {st} but no grammar is set (DecoderEngine.set_grammar)")
            if st != -1 and not 0 <= st < g.n_state:
                raise ValueError(f"row {b}: grammar_state {st} outside [0, {g.n_state})")
            out[b] = st
        return out

    # ------------------------------------------------------------------ model(idx, past) surface
    def reset(self, batch: int, max_len: Optional[int] = None):
        with self._on_stream():
            check(self.lib.mgea_decoder_reset(self.h, int(batch), int(max_len or self.max_ctx), self._sp()))
        self._cur_batch = int(batch)
        self._epoch += 1
        self._len = 0

    def forward(self, idx: torch.Tensor, lens: Optional[torch.Tensor] = None, want_logits: bool = True):
        """Append idx [B,T] to the cache and run the blocks (GPTWithKV.forward, api_cache.py:87-106)."""
        if idx.dim() != 2:
            raise RuntimeError("idx must be [B, T]")
        B, T = idx.shape
        self._check_ids(idx)
        with self._on_stream():
            ids32 = idx.to(device=self.device, dtype=torch.int32).contiguous()
            lens32 = None if lens is None else lens.to(device=self.device, dtype=torch.int32).contiguous()
            logits = torch.empty(B, T, self.vocab, dtype=torch.float32, device=self.device) if want_logits else None
            check(self.lib.mgea_decoder_forward(self.h, ptr(ids32), ptr(lens32), B, T, ptr(logits), self._sp()))
        self._len += T
        return logits

    def step(self, ids_in: Optional[torch.Tensor], sampler: SamplerConfig, want_logits: bool = False):
        with self._on_stream():
            B = self._batch()
            ids32 = None if ids_in is None else ids_in.to(device=self.device, dtype=torch.int32).contiguous()
            out = torch.empty(B, dtype=torch.int32, device=self.device)
            logits = torch.empty(B, self.vocab, dtype=torch.float32, device=self.device) if want_logits else None
            check(self.lib.mgea_decoder_step(self.h, ptr(ids32), C.byref(sampler), ptr(out), ptr(logits), self._sp()))
        self._len += 1
        return out, logits

    def _batch(self):
        return self._cur_batch

    def context_lengths(self) -> torch.Tensor:
        with self._on_stream():
            out = torch.empty(self._cur_batch, dtype=torch.int32, device=self.device)
            check(self.lib.mgea_decoder_context_lengths(self.h, ptr(out), self._sp()))
        return out

    def kv_rows(self, layer: int, lens: Sequence[int]):
        """Test only (mgea_decoder_kv_pages): the cached K and V of layer `layer`, read back through the page table: a list over the
        rows b < len(lens) of (k, v) CPU tensors [lens[b], n_head, head_dim] in the pages' dtype (fp32, or fp16 on f16 engines)."""
        from . import ops
        info = (C.c_int64 * 4)()
        check(self.lib.mgea_decoder_kv_pages(self.h, int(layer), None, 0, None, info, self._sp()))
        n_pages, max_pages, eb, nbytes = (int(x) for x in info)
        with self._on_stream():
            image = torch.empty(nbytes // eb, dtype=torch.float16 if eb == 2 else torch.float32, device=self.device)
            table = torch.empty(self.max_batch * max_pages, dtype=torch.int32, device=self.device)
            check(self.lib.mgea_decoder_kv_pages(self.h, int(layer), ptr(image), nbytes, ptr(table), info, self._sp()))
        torch.cuda.synchronize(self.device)
        image, table = image.cpu(), table.cpu().view(self.max_batch, max_pages).numpy()
        dh = self.d_model // self.n_head
        return [ops.kv_pages_read(image, table, b, int(n), self.n_head, dh) for b, n in enumerate(lens)]

    # ------------------------------------------------------------------ sample_kvcache surface
    def generate(self, prompts, n_steps: int, temperature: float = 1.0, top_k: Optional[int] = 50,
                 top_p: Optional[float] = None, eos_id: int = -1, seed: int = 0, check_ids: bool = True,
                 repetition_penalty: Optional[float] = None) -> torch.Tensor:
        """Batched sample_kvcache (api_cache.py:159-184).  prompts: list of id lists (ragged ok) or
        an int tensor [B, Tp].  Returns int32 [B, n_steps] of generated ids (-1 after a row's EOS).
        check_ids: prompts given as a DEVICE tensor are range-checked through the device flag once the
        generation has been enqueued (one sync at the end, which the caller's read of the ids needs anyway);
        False skips even that and leaves the flag for id_errors().
        repetition_penalty: None (or 1.0) = none; else a finite p > 0 (ValueError otherwise) applied like
        transformers' RepetitionPenaltyLogitsProcessor to every id of the row's prompt and of what it generated
        (mgea_decoder_generate_penalized); presence() then returns those sets.  (generate_biased: the same with a logit bias.)"""
        from . import ops
        pen = ops.check_repetition_penalty(repetition_penalty)
        ids, lens = _prompt_ids(prompts)
        B, Tp = ids.shape
        checked = self._check_ids(ids)
        samp = self.sampler(temperature, top_k, top_p, eos_id, seed)
        with self._on_stream():
            ids = ids.to(self.device).contiguous()
            lens = None if lens is None else lens.to(self.device).contiguous()
            out = torch.empty(B, max(n_steps, 1), dtype=torch.int32, device=self.device)
            if pen is None:
                check(self.lib.mgea_decoder_generate(self.h, ptr(ids), ptr(lens), B, Tp, int(n_steps), C.byref(samp), ptr(out),
                                                     self._sp()))
            else:
                check(self.lib.mgea_decoder_generate_penalized(self.h, ptr(ids), ptr(lens), B, Tp, int(n_steps), C.byref(samp),
                                                               pen, ptr(out), self._sp()))
        self._cur_batch = B
        self._epoch += 1
        if check_ids and not checked:
            self.id_errors()
        return out[:, :n_steps]

    def generate_biased(self, prompts, n_steps: int, temperature: float = 1.0, top_k: Optional[int] = 50,
                        top_p: Optional[float] = None, eos_id: int = -1, seed: int = 0, check_ids: bool = True,
                        repetition_penalty: Optional[float] = None, logit_bias=None, min_new_tokens: int = 0,
                        check_bias: bool = True) -> torch.Tensor:
        """generate() with a logit bias and a minimum length (generate()'s own parameter list is kept as it is).
        logit_bias: None, or one vector for all rows (a dict id -> bias, a host array or a device tensor [vocab]), or [B, vocab]:
        added to the penalized logits at every step, -inf bans an id.  min_new_tokens > 0 bans eos_id until a row has produced that
        many ids.  With either one this is generate_rows() with the same record on every row (stream = the row's index): the
        draws of generate(); with neither it IS generate().  check_bias=False skips the read-back that validates a DEVICE bias
        (check_logit_bias)."""
        from . import ops
        if logit_bias is None and int(min_new_tokens) == 0:
            return self.generate(prompts, n_steps, temperature, top_k, top_p, eos_id, seed, check_ids, repetition_penalty)
        pen = ops.check_repetition_penalty(repetition_penalty)
        B = prompts.shape[0] if isinstance(prompts, torch.Tensor) else len(prompts)
        per_row = [logit_bias] * B
        if not isinstance(logit_bias, dict) and logit_bias is not None and getattr(logit_bias, "ndim", 1) == 2:
            if logit_bias.shape[0] != B:
                raise ValueError(f"logit_bias must be [{self.vocab}] or [{B}, {self.vocab}], got {list(logit_bias.shape)}")
            per_row = [logit_bias[b] for b in range(B)]
        rows = [RowSampling(temperature, top_k, top_p, pen, eos_id, 0, seed, None, per_row[b], int(min_new_tokens))
                for b in range(B)]
        return self.generate_rows(prompts, rows, n_steps, check_ids, check_bias)

    def generate_rows(self, prompts, rows: Sequence[RowSampling], n_steps: Optional[int] = None,
                      check_ids: bool = True, check_bias: bool = True) -> torch.Tensor:
        """generate() with one RowSampling per prompt (mgea_decoder_generate_rows): concurrent requests with their own temperature,
        top-k, top-p, repetition penalty, EOS id, seed, Philox stream and step budget in one batch.  n_steps None = the largest
        max_new_tokens (every row then needs one > 0).  Returns int32 [B, n_steps]; -1 after a row's EOS or budget.  A row's ids
        depend on its prompt, its record and B, not on its index or on the other rows; with stream = b and no budget on every row
        this is generate().  Each row needs len(prompt) + its budget <= max_ctx: a row that would run past the context reserved
        for the batch, min(longest prompt + n_steps, max_ctx), finishes there.
        Rows with a logit_bias or min_new_tokens make it mgea_decoder_generate_rows_biased (the order of the processing steps and the
        validity rules: include/mgea.h); with none set this is the call it always was."""
        rows = list(rows)
        ids, lens = _prompt_ids(prompts)
        B, Tp = ids.shape
        if len(rows) != B:
            raise ValueError(f"{B} prompts but {len(rows)} sampler rows")
        n_steps = self._resolve_n_steps(rows, n_steps)
        return self._run_rows(ids, lens, rows, n_steps, check_ids=check_ids, check_bias=check_bias).ids

    @staticmethod
    def _resolve_n_steps(rows, n_steps: Optional[int]) -> int:
        """n_steps, or for None the largest max_new_tokens of the rows (every row then needs one > 0)."""
        if n_steps is None:
            budgets = [int(r.max_new_tokens) for r in rows]
            if min(budgets) <= 0:
                raise ValueError("n_steps=None needs max_new_tokens > 0 on every row")
            n_steps = max(budgets)
        return int(n_steps)

    def _run_rows(self, ids, lens, rows, n_steps: int, force_ids=None, scored: bool = False, guide=None, srecs=None,
                  n_seg_max: int = 1, check_ids: bool = True, check_bias: bool = True, blend=None) -> ScoredGeneration:
        """What generate_rows, generate_scored, generate_guided and generate_scheduled share: ids [B, Tp] (scheduled: [n_seg_max, B,
        Tp]) and lens from _prompt_ids, one RowSampling per row of B.  Packs the rows' records, logit records, forced ids and grammar
        start states (their ValueErrors, in that order), uploads on the engine's stream and makes the native call -- always
        mgea_decoder_generate_rows_scheduled, the superset, with NULL for what the caller does not use: it then runs exactly what
        the narrower entry point would -- or, when a row carries a Truncation, mgea_decoder_generate_rows_truncated, the same call
        with the rows' truncation records, or, with blend records, mgea_decoder_generate_rows_blended, or, when a row carries a
        ClassPenalty that is on, mgea_decoder_generate_rows_class_penalized, the end of the chain.
        Returns all B rows [B, n_steps]; logprobs / choice_logprobs are None unless scored."""
        B, Tp = ids.shape[-2:]
        recs = pack_rows(rows, self.vocab, n_steps)
        forced = pack_force_ids(force_ids, B, n_steps, self.vocab)
        lrecs, keep = pack_row_logits(rows, self.vocab, self.device, check_bias)
        starts = self._start_states(rows)
        trecs = pack_truncation(rows)
        crecs = pack_class_penalty(rows, n_steps, self._cpen_n_class)
        checked = self._check_ids(ids) and (forced is None or not forced.is_cuda)
        with self._on_stream():
            ids = ids.to(self.device).contiguous()
            lens = None if lens is None else lens.to(self.device).contiguous()
            forced = None if forced is None or n_steps == 0 else forced.to(self.device).contiguous()
            if forced is not None:   # a device matrix was packed on the caller's stream and is read by the engine's
                forced.record_stream(self.stream)
            w = max(n_steps, 1)
            out = torch.empty(B, w, dtype=torch.int32, device=self.device)
            lp = torch.zeros(B, w, dtype=torch.float32, device=self.device) if scored else None
            ch = torch.zeros(B, w, dtype=torch.float32, device=self.device) if scored else None
            for t in keep:   # uploaded on the caller's stream, read by the engine's
                t.record_stream(self.stream)
            if crecs is not None:
                check(self.lib.mgea_decoder_generate_rows_class_penalized(self.h, ptr(ids), ptr(lens), B, Tp, n_steps, recs, lrecs, starts,
                                                                          guide, srecs, n_seg_max, ptr(forced), ptr(out), ptr(lp), ptr(ch),
                                                                          trecs, blend, crecs, self._sp()))
            elif blend is not None:
                check(self.lib.mgea_decoder_generate_rows_blended(self.h, ptr(ids), ptr(lens), B, Tp, n_steps, recs, lrecs, starts, guide,
                                                                  srecs, n_seg_max, ptr(forced), ptr(out), ptr(lp), ptr(ch), trecs, blend,
                                                                  self._sp()))
            elif trecs is None:
                check(self.lib.mgea_decoder_generate_rows_scheduled(self.h, ptr(ids), ptr(lens), B, Tp, n_steps, recs, lrecs, starts, guide,
                                                                    srecs, n_seg_max, ptr(forced), ptr(out), ptr(lp), ptr(ch), self._sp()))
            else:
                check(self.lib.mgea_decoder_generate_rows_truncated(self.h, ptr(ids), ptr(lens), B, Tp, n_steps, recs, lrecs, starts, guide,
                                                                    srecs, n_seg_max, ptr(forced), ptr(out), ptr(lp), ptr(ch), trecs,
                                                                    self._sp()))
        self._cur_batch = B
        self._epoch += 1
        if check_ids and not checked:
            self.id_errors()
        return ScoredGeneration(out[:, :n_steps], lp[:, :n_steps] if scored else None, ch[:, :n_steps] if scored else None)

    def generate_scored(self, prompts, rows: Sequence[RowSampling], n_steps: Optional[int] = None, force_ids=None,
                        check_ids: bool = True, check_bias: bool = True) -> ScoredGeneration:
        """generate_rows() that also returns how likely every id was (mgea_decoder_generate_rows_scored; build-defined, the
        reference returns no scores).  logprobs: log-softmax of the RAW head logits at the id -- a function of the model alone;
        choice_logprobs: the id's log-probability under the distribution the draw was made from (after penalty, bias, temperature,
        top-k, top-p), -inf for a forced id outside the kept set, 0 for a greedy row.  force_ids (pack_force_ids: id lists, ragged
        allowed, or an int tensor; -1 = free) replace the drawn ids step by step -- a forced prefix, or teacher forcing (score()).
        The ids of the free steps are those of generate_rows(); all-greedy rows run as top_k = 1 rows of the sampled form."""
        rows = list(rows)
        ids, lens = _prompt_ids(prompts)
        B, Tp = ids.shape
        if len(rows) != B:
            raise ValueError(f"{B} prompts but {len(rows)} sampler rows")
        n_steps = self._resolve_n_steps(rows, n_steps)
        return self._run_rows(ids, lens, rows, n_steps, force_ids, True, check_ids=check_ids, check_bias=check_bias)

    def generate_guided(self, prompts, negative_prompts, rows: Sequence[RowSampling], guidance_scale=1.5,
                        n_steps: Optional[int] = None, force_ids=None, scored: bool = False, check_ids: bool = True,
                        check_bias: bool = True, all_rows: bool = False):
        """generate_rows() under classifier-free guidance (mgea_decoder_generate_rows_guided; build-defined, HuggingFace's
        guidance_scale).  negative_prompts[i] (id list, or None = row i is not guided) is prompt i without its conditioning tokens;
        the engine runs it as a shadow row behind the callers' rows, and at every step the pair draws ONE id from
        scale * logp(prompt) + (1 - scale) * logp(negative prompt): scale 1 = the conditional distribution, > 1 follows the
        conditioning more strongly, 0 = the negative prompt's.  guidance_scale: one value or one per prompt.  The mix comes before
        the repetition penalty (over the CONDITIONAL prompt and the generated ids), the bias and the grammar, which are row i's.
        A pair costs two rows of max_batch and one more launch per step; a call without any negative prompt is generate_rows /
        generate_scored itself.  Returns the callers' rows only: int32 [n, n_steps], or with scored=True a ScoredGeneration whose
        logprobs of a guided row are those of the guided distribution; all_rows=True returns the shadow rows too, behind the callers'
        rows in the order of their conditional rows (pack_guided).  force_ids as in generate_scored (scored=True only).
        ValueError naming the row for what the native call would refuse, a batch beyond max_batch and a capped generation
        (prompt width + n_steps > max_ctx without a window) included."""
        n = prompts.shape[0] if isinstance(prompts, torch.Tensor) else len(prompts)
        if force_ids is not None and not scored:
            raise ValueError("force_ids need scored=True")
        all_prompts, rows_all, shadow, scales, forced_in = pack_guided(prompts, negative_prompts, rows, guidance_scale, self.max_batch,
                                                                       force_ids)
        if all(u < 0 for u in shadow):   # nothing is guided: the calls there always were
            if scored:
                return self.generate_scored(prompts, rows, n_steps, force_ids, check_ids, check_bias)
            return self.generate_rows(prompts, rows, n_steps, check_ids, check_bias)
        ids, lens = _prompt_ids(all_prompts)
        B, Tp = ids.shape
        n_steps = self._resolve_n_steps(rows_all, n_steps)
        if self.window is None and Tp + n_steps > self.max_ctx:
            raise ValueError(f"prompt width {Tp} + {n_steps} steps exceed max_ctx {self.max_ctx}: a guided generation is never capped "
                             "(set a window)")
        guide = (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in zip(shadow, scales)])
        got = self._run_rows(ids, lens, rows_all, n_steps, forced_in, scored, guide, check_ids=check_ids, check_bias=check_bias)
        return got.first_rows(B if all_rows else n, scored)

    def generate_blended(self, prompt_groups, weights, rows: Sequence[RowSampling], n_steps: Optional[int] = None, force_ids=None,
                         scored: bool = False, check_ids: bool = True, check_bias: bool = True, all_rows: bool = False):
        """generate_rows() whose rows are emotion blends (mgea_decoder_generate_rows_blended; build-defined).  prompt_groups[i]: 1 to
        BLEND_MAX_ROWS prompts -- the same request conditioned on another emotion each --, weights[i]: one finite weight per prompt,
        summing to 1.  The engine runs the group as that many rows (its first prompt at row i, the others behind the callers' rows)
        and at every step the group draws ONE id from sum_k w_k * logp(prompt k), renormalised; the mix comes before the repetition
        penalty (over the FIRST prompt and the generated ids), the bias, the grammar and the truncation rules, which are row i's.
        A group of K prompts costs K rows of max_batch and one more launch per step; a call in which every group has one prompt is
        generate_rows / generate_scored itself.  Returns the leaders' lines only: int32 [n, n_steps], or with scored=True a
        ScoredGeneration whose logprobs are those of the blended distribution; all_rows=True returns the members too (pack_blended).
        force_ids as in generate_scored (scored=True only).  ValueError naming the row or group for what the native call would
        refuse, a batch beyond max_batch and a capped generation (prompt width + n_steps > max_ctx without a window) included."""
        if force_ids is not None and not scored:
            raise ValueError("force_ids need scored=True")
        all_prompts, rows_all, leader, weight, forced_in = pack_blended(prompt_groups, weights, rows, self.max_batch, force_ids)
        n = len(leader) - sum(1 for b, l in enumerate(leader) if l >= 0 and l != b)
        if all(l < 0 for l in leader):   # nothing is blended: the calls there always were
            if scored:
                return self.generate_scored(all_prompts, rows_all, n_steps, force_ids, check_ids, check_bias)
            return self.generate_rows(all_prompts, rows_all, n_steps, check_ids, check_bias)
        ids, lens = _prompt_ids(all_prompts)
        B, Tp = ids.shape
        n_steps = self._resolve_n_steps(rows_all, n_steps)
        if self.window is None and Tp + n_steps > self.max_ctx:
            raise ValueError(f"prompt width {Tp} + {n_steps} steps exceed max_ctx {self.max_ctx}: a blended generation is never capped "
                             "(set a window)")
        blend = (_lib.RowBlend * B)(*[_lib.RowBlend(leader=l, weight=w) for l, w in zip(leader, weight)])
        got = self._run_rows(ids, lens, rows_all, n_steps, forced_in, scored, check_ids=check_ids, check_bias=check_bias, blend=blend)
        return got.first_rows(B if all_rows else n, scored)

    def blend_info(self):
        """The groups, the grouped rows and the blended decode steps of the last generation (all 0 if it was not blended)."""
        out = (C.c_int64 * 3)()
        check(self.lib.mgea_decoder_blend_info(self.h, out))
        return dict(groups=int(out[0]), rows=int(out[1]), blended_steps=int(out[2]))

    def truncation_info(self):
        """The truncated decode steps of the last generation and its rows with a truncation stage on (both 0 if it was not truncated)."""
        out = (C.c_int64 * 2)()
        check(self.lib.mgea_decoder_truncation_info(self.h, out))
        return {"steps": int(out[0]), "rows": int(out[1])}

    def guidance_info(self):
        """The guidance pairs and the guided decode steps of the last generation (both 0 if it was not guided)."""
        out = (C.c_int64 * 2)()
        check(self.lib.mgea_decoder_guidance_info(self.h, out))
        return dict(pairs=out[0], guided_steps=out[1])

    def generate_scheduled(self, prompt_segments, rows: Sequence[RowSampling], schedules, n_steps: Optional[int] = None,
                           scored: bool = False, force_ids=None, negative_prompts=None, guidance_scale=1.5, check_ids: bool = True,
                           check_bias: bool = True):
        """generate_rows() whose rows change their prompt in the middle of the generation (mgea_decoder_generate_rows_scheduled;
        build-defined, the contract: include/mgea.h at mgea_row_schedule).  prompt_segments[b]: row b's prompt variants, id lists of
        one length (a bare id list = one variant); schedules[b]: its RowSchedule (None = a plain row).  At the start of every step a
        row whose segment (RowSchedule.segment_at of its step index or grammar state) has changed gets the K | V of the new variant
        over its prompt's cache positions; everything else of the row stays.  negative_prompts / guidance_scale as in
        generate_guided: the shadow rows are plain rows.  A call in which no row has more than one segment is generate_guided /
        generate_scored / generate_rows itself.  Returns the callers' rows: int32 [n, n_steps] or, scored, a ScoredGeneration.
        ValueError naming the row for what the native call would refuse."""
        rows = list(rows)
        n = len(rows)
        if force_ids is not None and not scored:
            raise ValueError("force_ids need scored=True")
        variants, scheds, n_seg_max = pack_scheduled(prompt_segments, schedules, rows, self.max_batch)
        if n_seg_max == 1:   # nothing is scheduled: the calls there always were
            return self.generate_guided(variants[0], negative_prompts, rows, guidance_scale, n_steps, force_ids, scored, check_ids,
                                        check_bias)
        all_prompts, rows_all, shadow, scales, forced_in = pack_guided(variants[0], negative_prompts, rows, guidance_scale,
                                                                       self.max_batch, force_ids)
        B = len(all_prompts)
        for u in range(n, B):   # a shadow row has one variant: its negative prompt in every segment
            if len(all_prompts[u]) > KV_PAGE_TOKENS:
                raise ValueError(f"row {u}: a negative prompt of {len(all_prompts[u])} tokens exceeds one page of {KV_PAGE_TOKENS}")
        scheds = scheds + [RowSchedule()] * (B - n)
        segs = []
        lens = None
        for s in range(n_seg_max):
            ids_s, lens = _prompt_ids(variants[s] + all_prompts[n:])
            segs.append(ids_s)
        ids = torch.stack(segs, dim=0).contiguous()   # [n_seg_max, B, Tp]: the variants of a row have one length, so one lens vector
        Tp = ids.shape[2]
        if Tp > KV_PAGE_TOKENS:
            raise ValueError(f"prompt width {Tp} exceeds one page of {KV_PAGE_TOKENS} tokens")
        n_steps = self._resolve_n_steps(rows_all, n_steps)
        guided = any(u >= 0 for u in shadow)
        if self.window is not None:
            self.window.check_call(Tp, n_steps)
        elif guided and Tp + n_steps > self.max_ctx:
            raise ValueError(f"prompt width {Tp} + {n_steps} steps exceed max_ctx {self.max_ctx}: a guided generation is never capped "
                             "(set a window)")
        guide = (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in zip(shadow, scales)]) if guided else None
        srecs = (_lib.RowSchedule * B)(*[s.record() for s in scheds])
        got = self._run_rows(ids, lens, rows_all, n_steps, forced_in, scored, guide, srecs, n_seg_max, check_ids, check_bias)
        return got.first_rows(n, scored)

    def schedule_info(self):
        """The scheduled decode steps and the switches (rows x times a row's prompt K | V was replaced) of the last generation, both 0
        if it was not scheduled (one stream sync)."""
        out = (C.c_int64 * 2)()
        with self._on_stream():
            check(self.lib.mgea_decoder_schedule_info(self.h, out, self._sp()))
        return dict(scheduled_steps=out[0], switches=out[1])

    def segments(self) -> torch.Tensor:
        """int32 [B] on the device: every row's segment after the last scheduled generation (shadow rows behind the callers' rows)."""
        with self._on_stream():
            out = torch.empty(self._cur_batch, dtype=torch.int32, device=self.device)
            check(self.lib.mgea_decoder_segments(self.h, ptr(out), self._sp()))
        return out

    def score(self, prompts, continuations, rows: Optional[Sequence[RowSampling]] = None):
        """Log-probabilities of given continuations under the model, as sample_kvcache would see them: a teacher-forced
        generate_scored() (prefill, re-feed the last prompt token, then every step takes continuations[b][t] instead of its draw --
        one prefill cannot do this, it is bidirectional).  continuations: B non-empty id lists (ragged allowed); row b runs
        len(continuations[b]) steps.  rows: None = greedy records with eos_id = -1 (the raw values do not depend on them); records
        of your own keep their settings but get that budget.  Returns (logprobs float32 [B, Tc] on the device, 0 past a row's
        length; their per-row sums [B])."""
        conts = [list(c) for c in continuations]
        if not conts or min(len(c) for c in conts) < 1:
            raise ValueError("empty continuation")
        if rows is None:
            rows = [RowSampling(top_k=1, eos_id=-1) for _ in conts]
        rows = list(rows)
        if len(rows) != len(conts):
            raise ValueError(f"{len(conts)} continuations but {len(rows)} sampler rows")
        rows = [dataclasses.replace(r, max_new_tokens=len(c)) for r, c in zip(rows, conts)]
        res = self.generate_scored(prompts, rows, max(len(c) for c in conts), force_ids=conts)
        return res.logprobs, res.logprobs.sum(dim=1)

    def score_prefill(self, prompts, continuations):
        """score() in ONE causal prefill per chunk of rows instead of one decode step per token; causal engines only (ValueError
        otherwise: a prefill of any other mode is bidirectional).  Resets, forwards prompt | continuation with logits and gathers the
        log-probability of token t + 1 from the logits at position t (mgea_op_logprob_gather).  The batch rows are chunked so that a
        chunk's logits buffer [rows, T, vocab] fp32 stays under SCORE_PREFILL_LOGITS_BYTES (256 MiB; one row at least) and under
        max_batch rows.  prompts and continuations: B non-empty id lists each (ragged allowed).  Returns what score() returns:
        (raw logprobs float32 [B, Tc] on the device, 0 past a row's length; their per-row sums [B]).
        One forward takes at most seq_len tokens per row (the position table; mgea_decoder_forward refuses more), while decode steps
        clamp positions and run on to max_ctx: a call with a row of more than seq_len tokens is scored by score(), step by step."""
        from . import ops
        if not self.causal:
            raise ValueError("score_prefill needs a pos_mode='causal' engine (any other prefill is bidirectional); use score()")
        prompts, conts = [list(p) for p in prompts], [list(c) for c in continuations]
        if not conts or len(prompts) != len(conts):
            raise ValueError(f"{len(prompts)} prompts but {len(conts)} continuations")
        if min(len(p) for p in prompts) < 1:
            raise ValueError("empty prompt")
        if min(len(c) for c in conts) < 1:
            raise ValueError("empty continuation")
        if max(len(p) + len(c) for p, c in zip(prompts, conts)) > self.seq_len:
            return self.score(prompts, conts)
        B, Tc = len(conts), max(len(c) for c in conts)
        out = torch.zeros(B, Tc, dtype=torch.float32, device=self.device)
        b0 = 0
        while b0 < B:
            # rows of this chunk: as many as the cap allows at the width of the chunk's first row (widths only shrink the count)
            n, T = 0, 0
            while b0 + n < B and n < self.max_batch:
                Tn = max(T, len(prompts[b0 + n]) + len(conts[b0 + n]))
                if n > 0 and (n + 1) * Tn * self.vocab * 4 > self.SCORE_PREFILL_LOGITS_BYTES:
                    break
                n, T = n + 1, Tn
            rows = [prompts[b] + conts[b] for b in range(b0, b0 + n)]
            ids, lens = _prompt_ids(rows)
            # targets[b, t] = the token at t + 1 where that is a continuation token, -1 (not scored) elsewhere
            tg = torch.full((n, T), -1, dtype=torch.int32)
            for i, b in enumerate(range(b0, b0 + n)):
                lp, lc = len(prompts[b]), len(conts[b])
                tg[i, lp - 1:lp - 1 + lc] = torch.tensor(conts[b], dtype=torch.int32)
            self._check_ids(ids)
            self.reset(n, T)
            logits = self.forward(ids, lens)
            with self._on_stream():
                lp_all = ops.logprob_gather(logits.view(n * T, self.vocab), tg.view(-1).to(self.device)).view(n, T)
                for i, b in enumerate(range(b0, b0 + n)):
                    lp, lc = len(prompts[b]), len(conts[b])
                    out[b, :lc] = lp_all[i, lp - 1:lp - 1 + lc]
            b0 += n
        return out, out.sum(dim=1)

    def presence(self) -> torch.Tensor:
        """bool [B, vocab] on the device: the ids each row of the last (penalized) generate() has seen -- its real prompt
        tokens and the ids it generated, EOS included.  RuntimeError if that generate() applied no penalty."""
        from . import ops
        with self._on_stream():
            words = torch.empty(self._cur_batch, ops.presence_words(self.vocab), dtype=torch.int32, device=self.device)
            check(self.lib.mgea_decoder_presence(self.h, ptr(words), self._sp()))
            return ops.unpack_presence(words, self.vocab)

    def reset_and_prefill(self, idx: torch.Tensor, lens=None, want_logits=True, max_len=None):
        self.reset(idx.shape[0], max_len)
        return self.forward(idx, lens, want_logits)

    PROFILE_CLASSES = ("gemm", "rowop", "attn_paged", "attn_dense", "sample")

    def profile(self, stride: int):
        """Time every `stride`-th decode step of generate() eagerly with HIP events (0 = off)."""
        check(self.lib.mgea_decoder_profile(self.h, int(stride)))

    def profile_read(self):
        ms = (C.c_double * 8)()
        n = (C.c_int64 * 8)()
        check(self.lib.mgea_decoder_profile_read(self.h, ms, n, 8))
        return {k: dict(ms=ms[i], launches=n[i]) for i, k in enumerate(self.PROFILE_CLASSES)}

    def stats(self):
        out = (C.c_int64 * 8)()
        check(self.lib.mgea_decoder_stats(self.h, out))
        tab = C.c_int64(0)
        check(self.lib.mgea_decoder_qkv0_table_bytes(self.h, C.byref(tab)))
        return dict(graph_nodes=out[0], graph_replays=out[1], graph_instantiates=out[2], graphs_cached=out[4], prefill16_forwards=out[5],
                    penalized_steps=out[6], biased_steps=out[7], scored_steps=out[3], qkv0_table_bytes=tab.value)
