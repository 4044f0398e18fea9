"""Host side of the MI355X decoder engine: weight arena, handle lifetime, torch tensor plumbing.

PyTorch is used only for device memory, streams and (in mgea.dist) the RCCL broadcast; all
arithmetic happens in libmgea_hip.so.  Mirrors GPTWithKV / sample_kvcache of the reference
(api_cache.py:76-106, 159-184) -- see generate_music/generate.py for the drop-in names.
The per-row records, their host models and the pack_* / check_* functions live in mgea.rows (no device in them); every name
of theirs is imported back here, where callers have always found it.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import DecoderConfig, SamplerConfig, check, ptr
from .rows import (BLEND_MAX_ROWS, CLASS_PENALTY_MAX_VALUE, CLASS_PENALTY_MAX_WINDOW, ERR_GRAMMAR_BANNED, ERR_ID_CLAMPED,  # noqa: F401
                   GRAMMAR_MAX_CELLS, GRAMMAR_MAX_CLASSES, GRAMMAR_MAX_STATES, KV_PAGE_TOKENS, SCHEDULE_MAX_SEGMENTS, WINDOW_MAX_RING,
                   WINDOW_MAX_STEPS, ClassPenalty, KVWindow, RowSampling, RowSchedule, ScoredGeneration, TokenGrammar, Truncation,
                   check_blend, check_guidance, check_logit_bias, dense_logit_bias, pack_blended, pack_class_penalty, pack_force_ids,
                   pack_guided, pack_row_logits, pack_rows, pack_scheduled, pack_truncation, split_logit_bias)

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
    cfg = DecoderConfig(vocab=geometry["vocab"], seq_len=geometry["seq_len"], d_model=geometry["d_model"],
                        n_head=n_head, n_layer=geometry["n_layer"], d_ff=geometry["d_ff"], max_batch=1, max_ctx=1,
                        dtype=_lib.DTYPE_F32, block_mode=0, pos_mode=0, ln_eps=1e-5)
    return _arena_layout(_lib.load(), cfg)


def _arena_layout(lib, cfg: DecoderConfig):
    """mgea_decoder_arena_layout for a config: once for the tensor count, once for the offsets"""
    n, total = C.c_int32(0), C.c_int64(0)
    check(lib.mgea_decoder_arena_layout(C.byref(cfg), None, C.byref(n), C.byref(total)))
    offs = (C.c_int64 * n.value)()
    check(lib.mgea_decoder_arena_layout(C.byref(cfg), offs, C.byref(n), C.byref(total)))
    return list(offs), total.value


# training-checkpoint tensor-name suffixes of the matrices the fp16 mode stores in fp16 (everything else stays fp32)
F16_ROUNDED_KEYS = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight", "fc.weight",
                    "attn.in_proj_weight", "attn.out_proj.weight", "mlp.0.weight", "mlp.2.weight", "head.weight")


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
        self.offsets, self.arena_floats = _arena_layout(self.lib, self.cfg)
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

    def _info(self, reader, n: int, *tail, ctype=C.c_int64) -> List[int]:
        """What a native *_info or stats reader fills in: n figures of the handle and of its last generation"""
        out = (ctype * n)()
        check(reader(self.h, out, *tail))
        return [int(v) for v in out]

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
        return dict(zip(("n_state", "n_class", "uploads", "grammar_steps"), self._info(self.lib.mgea_decoder_grammar_info, 4)))

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
        return dict(zip(("n_class", "rows", "class_penalized_steps"), self._info(self.lib.mgea_decoder_class_penalty_info, 3)))

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
        out = self._info(self.lib.mgea_decoder_window_info, 3, None, self._sp(), ctype=C.c_int32)
        return KVWindow(*out) if out[0] > 0 else None

    def window_evictions(self) -> List[int]:
        """The rows' eviction counts of the last generation (one stream sync); KVWindow.evictions is their closed form."""
        ev = (C.c_int32 * max(self._cur_batch, 1))()
        with self._on_stream():
            self._info(self.lib.mgea_decoder_window_info, 3, ev, self._sp(), ctype=C.c_int32)
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
        per_row = split_logit_bias(logit_bias, B, self.vocab)
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
        return self._run_rows([prompts], rows, n_steps, check_ids=check_ids, check_bias=check_bias).ids

    @staticmethod
    def _resolve_n_steps(rows, n_steps: Optional[int]) -> int:
        """n_steps, or for None the largest max_new_tokens of the rows (every row then needs one > 0)."""
        if n_steps is None:
            budgets = [int(r.max_new_tokens) for r in rows]
            if min(budgets) <= 0:
                raise ValueError("n_steps=None needs max_new_tokens > 0 on every row")
            n_steps = max(budgets)
        return int(n_steps)

    def _run_rows(self, segments, rows, n_steps: Optional[int], force_ids=None, scored: bool = False, check_ids: bool = True,
                  check_bias: bool = True, guidance=None, blend=None, schedules=None, never_capped: Optional[str] = None) -> ScoredGeneration:
        """The one path from every generate_* method to the native call.  segments: the whole batch's prompts (id lists, or an int
        tensor [B, Tp]) once per prompt segment -- one entry unless the call is scheduled; rows: one RowSampling per row of B.
        guidance (shadow_rows, scales), blend (leaders, weights) and schedules (one RowSchedule per row) are what pack_guided,
        pack_blended and pack_scheduled return for the whole batch, None = the call has none; never_capped ("guided" / "blended"):
        without a window such a generation is refused where prompt width + n_steps exceed max_ctx.
        Lays out the prompts, resolves n_steps (None = the largest max_new_tokens), checks the window or the cap, packs the rows'
        records, forced ids, logit records, grammar start states, truncation and class-penalty records (their ValueErrors, in that
        order), uploads on the engine's stream and makes ONE native call, mgea_decoder_generate_rows_class_penalized -- the end of
        the chain of entry points, with NULL for every record the call does not use: csrc/decoder_generate.hip builds the same
        request from it that the narrower entry point would (tests/test_gpu_generate_entry_points.py).
        Returns all B rows [B, n_steps]; logprobs / choice_logprobs are None unless scored."""
        rows = list(rows)
        laid = [_prompt_ids(p) for p in segments]
        lens = laid[-1][1]   # (the variants of a row have one length, so one lens vector)
        ids = laid[0][0] if len(laid) == 1 else torch.stack([i for i, _ in laid], dim=0).contiguous()   # [B, Tp] or [n_seg_max, B, Tp]
        B, Tp = ids.shape[-2:]
        if len(rows) != B:
            raise ValueError(f"{B} prompts but {len(rows)} sampler rows")
        if schedules is not None and Tp > KV_PAGE_TOKENS:
            raise ValueError(f"prompt width {Tp} exceeds one page of {KV_PAGE_TOKENS} tokens")
        n_steps = self._resolve_n_steps(rows, n_steps)
        if schedules is not None and self.window is not None:
            self.window.check_call(Tp, n_steps)
        elif never_capped and self.window is None and Tp + n_steps > self.max_ctx:
            raise ValueError(f"prompt width {Tp} + {n_steps} steps exceed max_ctx {self.max_ctx}: a {never_capped} generation is never "
                             "capped (set a window)")
        guide = guidance and (_lib.RowGuidance * B)(*[_lib.RowGuidance(shadow_row=u, scale=s) for u, s in zip(*guidance)])
        brecs = blend and (_lib.RowBlend * B)(*[_lib.RowBlend(leader=l, weight=w) for l, w in zip(*blend)])
        srecs = schedules and (_lib.RowSchedule * B)(*[s.record() for s in schedules])
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
            check(self.lib.mgea_decoder_generate_rows_class_penalized(self.h, ptr(ids), ptr(lens), B, Tp, n_steps, recs, lrecs, starts, guide,
                                                                      srecs, len(laid), ptr(forced), ptr(out), ptr(lp), ptr(ch), trecs, brecs,
                                                                      crecs, self._sp()))
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
        return self._run_rows([prompts], rows, n_steps, force_ids, True, check_ids, check_bias)

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
        got = self._run_rows([all_prompts], rows_all, n_steps, forced_in, scored, check_ids, check_bias, guidance=(shadow, scales),
                             never_capped="guided")
        return got.first_rows(len(all_prompts) if all_rows else n, scored)

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
        got = self._run_rows([all_prompts], rows_all, n_steps, forced_in, scored, check_ids, check_bias, blend=(leader, weight),
                             never_capped="blended")
        return got.first_rows(len(all_prompts) if all_rows else n, scored)

    def blend_info(self):
        """The groups, the grouped rows and the blended decode steps of the last generation (all 0 if it was not blended)."""
        return dict(zip(("groups", "rows", "blended_steps"), self._info(self.lib.mgea_decoder_blend_info, 3)))

    def truncation_info(self):
        """The truncated decode steps of the last generation and its rows with a truncation stage on (both 0 if it was not truncated)."""
        return dict(zip(("steps", "rows"), self._info(self.lib.mgea_decoder_truncation_info, 2)))

    def guidance_info(self):
        """The guidance pairs and the guided decode steps of the last generation (both 0 if it was not guided)."""
        return dict(zip(("pairs", "guided_steps"), self._info(self.lib.mgea_decoder_guidance_info, 2)))

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
        guided = any(u >= 0 for u in shadow)
        got = self._run_rows([v + all_prompts[n:] for v in variants], rows_all, n_steps, forced_in, scored, check_ids, check_bias,
                             guidance=(shadow, scales) if guided else None, schedules=scheds + [RowSchedule()] * (B - n),
                             never_capped="guided" if guided else None)
        return got.first_rows(n, scored)

    def schedule_info(self):
        """The scheduled decode steps and the switches (rows x times a row's prompt K | V was replaced) of the last generation, both 0
        if it was not scheduled (one stream sync)."""
        with self._on_stream():
            return dict(zip(("scheduled_steps", "switches"), self._info(self.lib.mgea_decoder_schedule_info, 2, self._sp())))

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
        out = self._info(self.lib.mgea_decoder_stats, 8)
        tab = C.c_int64(0)
        check(self.lib.mgea_decoder_qkv0_table_bytes(self.h, C.byref(tab)))
        return dict(graph_nodes=out[0], graph_replays=out[1], graph_instantiates=out[2], graphs_cached=out[4], prefill16_forwards=out[5],
                    penalized_steps=out[6], biased_steps=out[7], scored_steps=out[3], qkv0_table_bytes=tab.value)
