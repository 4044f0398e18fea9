"""Drop-in for the decoder half of the reference: the names `api_cache.py` defines for itself
(`GPTWithKV`, `remap_state_dict`, `sample_kvcache`, `encode`, `decode`, `closest_bpm_token`,
`normalize_key_signature`, `FAMILY_TO_INSTRUMENTS`, `note_re`; api_cache.py:76-184) and the ones
`generate_music/generate.py` defines (`GPT`, `sample`; generate.py:25-61), plus the north-star name
`generate_sequence`.  Every tensor operation runs in libmgea_hip.so on the MI355X; importing this
module has no side effects (the reference's files load a checkpoint at import time).

Replacing api_cache.py:39-138,159-184 by

    from generate_music.generate import *          # GPTWithKV, remap_state_dict, sample_kvcache, ...
    model, tok2id, id2tok, SEQ_LEN, D_MODEL = load_checkpoint(CKPT)

leaves its endpoint (api_cache.py:186-243) untouched.

Note on the small host helpers: `FAMILY_TO_INSTRUMENTS`, `note_re`, `encode`, `decode`, `closest_bpm_token` and
`normalize_key_signature` below are the drop-in's constant table, one regex and four one-to-seven-line functions whose exact
behaviour (keys, error classes, string formats) IS the contract with api_cache.py:140-157 -- they are restated line for line
from there on purpose (each cites its lines); everything that computes (the model, the sampler loop) is this repo's own design.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence

import torch

from mgea.decoder import (DecoderEngine, RowSampling, Truncation, geometry_from_state_dict, remap_state_dict,  # noqa: F401
                          split_logit_bias)

__all__ = ["GPTWithKV", "GPT", "remap_state_dict", "load_checkpoint", "set_vocab", "encode", "decode",
           "closest_bpm_token", "normalize_key_signature", "FAMILY_TO_INSTRUMENTS", "note_re", "sample_kvcache",
           "generate_sequence", "generate_requests", "sample", "tok2id", "id2tok", "sample_kvcache_biased",
           "generate_batch_biased", "generate_sequence_biased", "sample_kvcache_grammar", "generate_batch_grammar", "sample_kvcache_truncated",
           "generate_sequence_truncated", "generate_batch_truncated", "score_sequence", "generate_best_of", "pick_best",
           "mean_logprobs", "sample_kvcache_guided", "generate_requests_guided", "sample_kvcache_blended", "generate_requests_blended",
           "sample_kvcache_varied"]

# module globals like the reference's (api_cache.py:34-35); filled by load_checkpoint / set_vocab
tok2id: Dict[str, int] = {}
id2tok: Dict[int, str] = {}
model = None  # generate.py's `sample(prompt, ...)` uses a module-level model

FAMILY_TO_INSTRUMENTS = {          # api_cache.py:152-156
    "Strings": ["Violin"],
    "Piano": ["Acoustic Grand Piano"],
    "Woodwind": ["Flute"],
}
note_re = re.compile(r"\[NOTE\] \[PITCH:(.+?)\] \[START:(.+?)\] \[END:(.+?)\] \[DURATION:(.+?)\]")  # api_cache.py:157

_DEFAULT_DEVICE = "cuda:0"


def set_vocab(vocab: Dict[str, int]) -> None:
    """Install the token<->id maps (api_cache.py:34-35)."""
    tok2id.clear()
    tok2id.update(vocab)
    id2tok.clear()
    id2tok.update({i: t for t, i in vocab.items()})


def encode(tokens):            # api_cache.py:140
    return torch.tensor([tok2id[t] for t in tokens])


def decode(ids):               # api_cache.py:141
    return [id2tok[int(i)] for i in ids]


def closest_bpm_token(val):    # api_cache.py:142-144 (ValueError from min() when no [BPM] token exists)
    bpm_toks = [t for t in tok2id if t.startswith("[BPM]")]
    return min(bpm_toks, key=lambda s: abs(float(s.split()[-1]) - val))


def normalize_key_signature(key_string):   # api_cache.py:145-151
    key_string = key_string.replace("♭", "-").replace("♯", "#")
    parts = key_string.strip().split()
    if len(parts) == 2:
        key, scale = parts
        return f"[KEY_SIGNATURE] {key} {scale.lower()}"
    return f"[KEY_SIGNATURE] {key_string}"


class _KVState(list):
    """What `model(idx, past)` returns as `presents`: the cache itself lives in the native engine's
    KV pages; this token only proves the caller continues the most recent sequence.  It is a list of
    n_layer entries so code that zips it with the layers (api_cache.py:101) still works."""

    def __init__(self, n_layer, epoch, length):
        super().__init__([None] * n_layer)
        self.epoch, self.length = epoch, length


class GPTWithKV:
    """Same constructor / call surface as the reference class (api_cache.py:76-106), backed by a
    native decoder handle.  Weights arrive through load_state_dict (names after remap_state_dict)."""

    block_mode = "kv"

    def __init__(self, vocab_size, seq_len, d_model, n_head, n_layer, max_batch: int = 8,
                 max_ctx: Optional[int] = None, device: str = _DEFAULT_DEVICE, dtype: str = "f32", causal: bool = False):
        self.vocab_size, self.seq_len, self.d_model = int(vocab_size), int(seq_len), int(d_model)
        self.n_head, self.n_layer = int(n_head), int(n_layer)
        self.max_batch, self.max_ctx, self.device = int(max_batch), max_ctx, device
        self.dtype = dtype   # "f32" = the reference's arithmetic (parity mode); "f16" = fp16 matrices + KV (mgea.decoder)
        # causal: a checkpoint trained WITH a causal mask (a standard GPT) -- true positions, masked prefill, every token fed once
        # (DecoderEngine pos_mode="causal"); False: the reference's model as api_cache.py evaluates it
        self.causal = bool(causal)
        self.engine: Optional[DecoderEngine] = None
        self._epoch = -1
        self._window = None   # set_window's arguments, applied to every engine load_state_dict builds

    # -- nn.Module look-alikes ----------------------------------------------------------------
    def load_state_dict(self, sd: Dict, strict: bool = True):
        sd = remap_state_dict(sd)
        geo = geometry_from_state_dict(sd)
        want = dict(vocab=self.vocab_size, seq_len=self.seq_len, d_model=self.d_model, n_layer=self.n_layer)
        for k, v in want.items():
            if geo[k] != v:   # what nn.Module.load_state_dict reports as a size mismatch
                raise RuntimeError(f"Error(s) in loading state_dict: size mismatch for {k}: checkpoint {geo[k]}, model {v}")
        if self.engine is not None:
            self.engine.close()
        max_ctx = self.max_ctx if self.max_ctx is not None else max(self.seq_len, 1)
        self.engine = DecoderEngine(sd, n_head=self.n_head, max_batch=self.max_batch, max_ctx=max_ctx,
                                    device=self.device, block_mode=self.block_mode, dtype=self.dtype,
                                    pos_mode="causal" if self.causal else "reference")
        if self._window is not None:
            self.engine.set_window(*self._window)
        return "<All keys matched successfully>"

    def set_window(self, sink_pages: int = 1, ring_pages: Optional[int] = None, max_steps: Optional[int] = None):
        """Give the model a KV window (DecoderEngine.set_window): sample_kvcache and the other generation calls then take a max_len
        beyond the engine's context -- the prompt stays cached, the oldest generated tokens leave a 64-token page at a time, as
        the reference's own loop has no context limit (api_cache.py:159-184).  sink_pages 0 clears it.  Kept across
        load_state_dict."""
        if self.causal and int(sink_pages) != 0:   # before any engine is built (load_checkpoint(window=, causal=True) ends here)
            raise ValueError("window: a causal model has no KV window (a step's position is its cached length); it needs causal=False")
        self._window = None if int(sink_pages) == 0 else (int(sink_pages), ring_pages, max_steps)
        if self.engine is not None:
            self.engine.set_window(sink_pages, ring_pages, max_steps)
        return self

    def eval(self):
        return self

    def to(self, device=None, *a, **k):
        return self  # the model lives on its MI355X; `device="cpu"` of the reference call is accepted and ignored

    def _need(self) -> DecoderEngine:
        if self.engine is None:
            raise RuntimeError("GPTWithKV has no weights: call load_state_dict first")
        return self.engine

    def __call__(self, idx: torch.Tensor, past_kv=None):
        """logits [B,T,V] (fp32, on the GPU) and an opaque `presents` to pass back as past_kv."""
        eng = self._need()
        B, T = idx.shape
        fresh = past_kv is None or (not isinstance(past_kv, _KVState) and all(p is None for p in past_kv))
        if fresh:   # api_cache.py:96-97: past_kv=None means an empty cache
            eng.reset(B)
            self._epoch = eng._epoch
        else:
            if not isinstance(past_kv, _KVState) or past_kv.epoch != self._epoch or past_kv.length != eng._len:
                raise RuntimeError("past_kv is not the most recent `presents` of this model "
                                   "(the KV cache lives in the native engine and only grows)")
        logits = eng.forward(idx, None, want_logits=True)
        return logits, _KVState(self.n_layer, self._epoch, eng._len)

    forward = __call__


class GPT(GPTWithKV):
    """The no-cache twin of generate_music/generate.py:25-35 (post-LN, ReLU nn.TransformerEncoder,
    full recompute, no mask): `model(x)` returns logits only.  Takes the training checkpoint as is."""

    block_mode = "twin"

    def __init__(self, vocab, seq_len, d_model, n_head=4, n_layer=2, **kw):
        # generate.py stores seq_len-1 position rows (generate.py:18,29)
        super().__init__(vocab, seq_len - 1, d_model, n_head, n_layer, **kw)

    def __call__(self, x: torch.Tensor):
        eng = self._need()
        return eng.reset_and_prefill(x, None, want_logits=True)

    forward = __call__


def load_checkpoint(path, n_head: int = 8, device: str = _DEFAULT_DEVICE, max_batch: int = 8,
                    max_ctx: Optional[int] = None, window=None, causal: bool = False):
    """api_cache.py:26-37,108-138 in one call: torch.load(weights_only=True), geometry from tensor
    shapes, GPTWithKV + remapped weights.  Returns (model, tok2id, id2tok, SEQ_LEN, D_MODEL) and
    installs the vocabulary in this module.  window (None, or (sink_pages, ring_pages[, max_steps])): GPTWithKV.set_window.
    causal=True: the checkpoint was trained with a causal mask; it is served as a standard causal GPT (GPTWithKV(causal=True))."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    geo = geometry_from_state_dict(ckpt["model"])
    set_vocab(ckpt["vocab"])
    m = GPTWithKV(vocab_size=len(tok2id), seq_len=geo["seq_len"], d_model=geo["d_model"], n_head=n_head,
                  n_layer=geo["n_layer"], max_batch=max_batch, max_ctx=max_ctx, device=device, causal=causal)
    if window is not None:
        m.set_window(*window)
    m.load_state_dict(remap_state_dict(ckpt["model"]))
    global model
    model = m
    return m, tok2id, id2tok, geo["seq_len"], geo["d_model"]


def _as_model(model_or_weights, n_head=8, device=_DEFAULT_DEVICE) -> GPTWithKV:
    if isinstance(model_or_weights, GPTWithKV):
        return model_or_weights
    if isinstance(model_or_weights, dict):
        sd = model_or_weights.get("model", model_or_weights)
        if "vocab" in model_or_weights and not tok2id:
            set_vocab(model_or_weights["vocab"])
        geo = geometry_from_state_dict(sd)
        m = GPTWithKV(geo["vocab"], geo["seq_len"], geo["d_model"], n_head, geo["n_layer"], device=device)
        m.load_state_dict(sd)
        return m
    raise TypeError("expected a GPTWithKV or a state dict / checkpoint dict")


def _no_window(eng) -> bool:
    """True when the engine stops a generation at its reserved context (no KV window: DecoderEngine.set_window)."""
    return getattr(eng, "window", None) is None


def _use_grammar(eng, grammar) -> None:
    """Make `grammar` (a TokenGrammar, or None = nothing to do) the engine's: uploaded when it is not the object set there now."""
    if grammar is not None and eng.grammar is not grammar:
        eng.set_grammar(grammar)


def _engine_generate(eng, ids, n_steps, logit_bias, min_new_tokens, grammar=None, truncation=None, **kw):
    """eng.generate(), or eng.generate_biased() when a bias or a minimum length is set (capped at the steps there are); with a
    grammar or a Truncation, generate_rows() with the same record on every row (stream = the row's index: the draws of generate())
    and, under a grammar, each row's start state walked from its prompt"""
    if grammar is not None or truncation is not None:
        from .grammar import start_state
        _use_grammar(eng, grammar)
        B = len(ids)
        per_row = split_logit_bias(logit_bias, B, eng.vocab)
        rows = [RowSampling(temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 50), top_p=kw.get("top_p"),
                            repetition_penalty=kw.get("repetition_penalty"), eos_id=kw.get("eos_id", -1), seed=kw.get("seed", 0),
                            logit_bias=per_row[b], min_new_tokens=min(int(min_new_tokens), n_steps),
                            grammar_state=None if grammar is None else start_state(grammar, ids[b]), truncation=truncation)
                for b in range(B)]
        return eng.generate_rows(ids, rows, n_steps)
    if logit_bias is None and not min_new_tokens:
        return eng.generate(ids, n_steps, **kw)
    return eng.generate_biased(ids, n_steps, logit_bias=logit_bias, min_new_tokens=min(int(min_new_tokens), n_steps), **kw)


def _draw_seed() -> int:
    # torch.manual_seed(s) therefore makes a sampled generation reproducible, like the reference
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def sample_kvcache(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                   top_p: Optional[float] = None, seed: Optional[int] = None,
                   repetition_penalty: Optional[float] = None) -> List[str]:
    """api_cache.py:159-184 with the same signature: prefill the prompt (logits dropped), then up to
    max_len - len(prompt) steps of /temperature, top-k mask, softmax, one multinomial draw; stops
    after [END_SEQUENCE].  Runs as one native generate() call (prefill + hipGraph-replayed decode
    steps).  `device` is accepted for compatibility; the work happens on the model's MI355X.
    top_k=1 is exactly greedy; other settings match torch.multinomial in distribution only.
    repetition_penalty (None = none) penalizes the ids of the prompt and of everything generated so far like
    transformers' RepetitionPenaltyLogitsProcessor; the paper's setting is top_k=0, top_p=0.92, repetition_penalty=1.1.
    (sample_kvcache_biased: the same with a logit bias and a minimum length.)"""
    return sample_kvcache_biased(model, prompt, max_len, temperature, top_k, device, top_p, seed, repetition_penalty)


def sample_kvcache_biased(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                          top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                          logit_bias=None, min_new_tokens: int = 0) -> List[str]:
    """sample_kvcache with a constraint on what may be drawn (sample_kvcache keeps the reference's parameter list).
    logit_bias (None, a dict id -> bias, a host array or a device tensor [vocab]; -inf bans an id -- generate_music.constraints
    builds the note / scale ones) is added to the penalized logits at every step; min_new_tokens > 0 keeps [END_SEQUENCE] from
    being drawn before that many new tokens (capped at the steps there are).  Both are build-defined (include/mgea.h); with
    neither this is sample_kvcache, the same engine call.  (sample_kvcache_grammar: the same with a token grammar.)"""
    return sample_kvcache_grammar(model, prompt, max_len, temperature, top_k, device, top_p, seed, repetition_penalty, logit_bias,
                                  min_new_tokens)


def sample_kvcache_grammar(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                           top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                           logit_bias=None, min_new_tokens: int = 0, grammar=None,
                           min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache_biased under a token grammar (sample_kvcache_biased keeps its parameter list).  grammar (a
    mgea.decoder.TokenGrammar, e.g. generate_music.grammar.track_grammar; None = none: then this IS sample_kvcache_biased)
    constrains what may FOLLOW what: the row starts in the state its prompt leads to (generate_music.grammar.start_state), every
    step is masked by the row's current state, and the state moves on the device.  It composes with logit_bias: the bias bans ids,
    the grammar orders the rest.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    m = _as_model(model)
    eng = m._need()
    ids = [tok2id[t] for t in prompt]          # KeyError for an unknown token, like api_cache.py:162
    n_steps = int(max_len) - len(ids)
    if n_steps <= 0:
        return [id2tok[i] for i in ids]
    if _no_window(eng) and len(ids) + n_steps > eng.max_ctx:
        raise RuntimeError(f"max_len={max_len} exceeds the engine's reserved context {eng.max_ctx}")
    eos = tok2id.get("[END_SEQUENCE]", -1)
    out = _engine_generate(eng, [ids], n_steps, logit_bias, min_new_tokens, grammar, temperature=temperature, top_k=top_k,
                           top_p=top_p, eos_id=eos, seed=_draw_seed() if seed is None else seed,
                           repetition_penalty=repetition_penalty,
                           truncation=Truncation.of(min_p, typical_p, epsilon_cutoff, eta_cutoff))
    gen = [int(i) for i in out[0].cpu().tolist() if i >= 0]
    return [id2tok[i] for i in ids + gen]


def generate_sequence(model_or_weights, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50,
                      device=_DEFAULT_DEVICE, top_p: Optional[float] = None, seed: Optional[int] = None,
                      n_head: int = 8, repetition_penalty: Optional[float] = None) -> List[str]:
    """North-star name (BASELINE.json): sample_kvcache on a model object or a weights/checkpoint dict."""
    return sample_kvcache(_as_model(model_or_weights, n_head, device), prompt, max_len, temperature, top_k,
                          device, top_p, seed, repetition_penalty=repetition_penalty)


def generate_sequence_biased(model_or_weights, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50,
                             device=_DEFAULT_DEVICE, top_p: Optional[float] = None, seed: Optional[int] = None, n_head: int = 8,
                             repetition_penalty: Optional[float] = None, logit_bias=None, min_new_tokens: int = 0) -> List[str]:
    """generate_sequence with a logit bias and a minimum length: sample_kvcache_biased on a model object or a weights dict."""
    return sample_kvcache_biased(_as_model(model_or_weights, n_head, device), prompt, max_len, temperature, top_k, device, top_p,
                                 seed, repetition_penalty, logit_bias, min_new_tokens)


def generate_batch(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                   top_p: Optional[float] = None, seed: Optional[int] = None,
                   repetition_penalty: Optional[float] = None) -> List[List[str]]:
    """New surface: many prompts in one batch (ragged lengths allowed); every row equals the
    reference run on that prompt alone (greedy) -- rows are independent."""
    return generate_batch_biased(model, prompts, max_len, temperature, top_k, top_p, seed, repetition_penalty)


def generate_batch_biased(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                          top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                          logit_bias=None, min_new_tokens: int = 0) -> List[List[str]]:
    """generate_batch with a logit bias (one vector for every row, or [B, vocab]) and min_new_tokens, as in sample_kvcache_biased."""
    return generate_batch_grammar(model, prompts, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias,
                                  min_new_tokens)


def generate_batch_grammar(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                           top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                           logit_bias=None, min_new_tokens: int = 0, grammar=None,
                           min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[List[str]]:
    """generate_batch_biased under a token grammar (None = none), as in sample_kvcache_grammar: every row starts in the state of its
    own prompt.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    m = _as_model(model)
    eng = m._need()
    ids = [[tok2id[t] for t in p] for p in prompts]
    n_steps = int(max_len) - max(len(p) for p in ids)
    eos = tok2id.get("[END_SEQUENCE]", -1)
    out = _engine_generate(eng, ids, max(n_steps, 0), logit_bias, min_new_tokens, grammar, temperature=temperature, top_k=top_k,
                           top_p=top_p, eos_id=eos, seed=_draw_seed() if seed is None else seed,
                           repetition_penalty=repetition_penalty,
                           truncation=Truncation.of(min_p, typical_p, epsilon_cutoff, eta_cutoff)).cpu().tolist()
    return [[id2tok[i] for i in p + [g for g in row if g >= 0]] for p, row in zip(ids, out)]


def sample_kvcache_truncated(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                             top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                             logit_bias=None, min_new_tokens: int = 0, grammar=None,
                             min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache with HuggingFace's further truncation rules (sample_kvcache and sample_kvcache_biased keep their parameter
    lists; sample_kvcache_grammar takes the same four keywords): min_p, typical_p (locally typical sampling), epsilon_cutoff and
    eta_cutoff, None = off, applied in this order behind top-k and top-p inside the engine's sampler (mgea.decoder.Truncation;
    build-defined, the reference has none).  With none of them this is sample_kvcache_grammar, the same engine call."""
    return sample_kvcache_grammar(model, prompt, max_len, temperature, top_k, device, top_p, seed, repetition_penalty, logit_bias,
                                  min_new_tokens, grammar,
                                  min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)


def generate_sequence_truncated(model_or_weights, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50,
                                device=_DEFAULT_DEVICE, top_p: Optional[float] = None, seed: Optional[int] = None, n_head: int = 8,
                                repetition_penalty: Optional[float] = None, logit_bias=None, min_new_tokens: int = 0, grammar=None,
                                min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """generate_sequence with the four truncation keywords: sample_kvcache_truncated on a model object or a weights dict."""
    return sample_kvcache_truncated(_as_model(model_or_weights, n_head, device), prompt, max_len, temperature, top_k, device, top_p,
                                    seed, repetition_penalty, logit_bias, min_new_tokens, grammar,
                                    min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)


def generate_batch_truncated(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                             top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                             logit_bias=None, min_new_tokens: int = 0, grammar=None,
                             min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[List[str]]:
    """generate_batch with the four truncation keywords of sample_kvcache_truncated, the same values on every row
    (generate_batch_grammar takes them too; generate_requests takes one value per prompt)."""
    return generate_batch_grammar(model, prompts, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias,
                                  min_new_tokens, grammar,
                                  min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)


def score_sequence(model, prompt_tokens: Sequence[str], continuation_tokens: Sequence[str]) -> List[float]:
    """The log-probability (natural log, raw head logits: no temperature, no top-k) of every token of continuation_tokens as
    sample_kvcache would come to it after prompt_tokens: a teacher-forced run of the decode steps (DecoderEngine.score) -- or, for a
    causal model, ONE masked prefill of prompt + continuation (DecoderEngine.score_prefill; beyond seq_len tokens, the position table,
    a causal model too is scored step by step).
    Build-defined -- the reference returns no scores.  sum() of the result is the continuation's log-likelihood, exp(-mean) its
    perplexity."""
    eng = _as_model(model)._need()
    ids = [tok2id[t] for t in prompt_tokens]          # KeyError for an unknown token, like api_cache.py:162
    cont = [tok2id[t] for t in continuation_tokens]
    if not cont:
        return []
    if _no_window(eng) and len(ids) + len(cont) > eng.max_ctx:
        raise RuntimeError(f"prompt + continuation = {len(ids) + len(cont)} tokens exceed the engine's reserved context {eng.max_ctx}")
    lp, _ = eng.score_prefill([ids], [cont]) if eng.causal else eng.score([ids], [cont])
    return [float(v) for v in lp[0].cpu().tolist()]


def mean_logprobs(ids, logprobs) -> List[float]:
    """Per candidate row: the mean raw log-probability over the ids the row produced (ids >= 0); -inf for a row that produced none.
    ids, logprobs: [n, steps] as nested lists or arrays on the host."""
    out = []
    for row_ids, row_lp in zip(ids, logprobs):
        kept = [float(v) for i, v in zip(row_ids, row_lp) if int(i) >= 0]
        out.append(sum(kept) / len(kept) if kept else float("-inf"))
    return out


def pick_best(ids, logprobs) -> int:
    """The candidate generate_best_of keeps: the row with the highest mean_logprobs, ties to the lowest index.  Pure host code."""
    means = mean_logprobs(ids, logprobs)
    best = 0
    for i, m in enumerate(means):
        if m > means[best]:
            best = i
    return best


def generate_best_of(model, prompt: Sequence[str], n: int, max_len=512, temperature=1.0, top_k=50, top_p: Optional[float] = None,
                     seed: Optional[int] = None, repetition_penalty: Optional[float] = None, logit_bias=None, min_new_tokens: int = 0,
                     return_all: bool = False, grammar=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """sample_kvcache_biased n times in ONE batch, keeping the most likely candidate: the n rows share the prompt, the settings and
    the seed and draw from Philox streams 0 .. n - 1 (row 0 is the sample_kvcache run of that seed); the one with the highest mean
    raw log-probability per generated token (pick_best) is returned as prompt + generated tokens.  n is capped by the model's
    max_batch (ValueError beyond it).  return_all=True returns (tokens, candidates, means, best): every candidate's tokens, their
    mean log-probabilities and the index kept.  grammar (a TokenGrammar or None): every candidate starts in the state of the prompt.
    Build-defined: the reference draws one sequence and returns no scores.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    m = _as_model(model)
    n = int(n)
    if n < 1 or n > m.max_batch:
        raise ValueError(f"best-of n={n} outside [1, max_batch={m.max_batch}]")
    eng = m._need()
    ids = [tok2id[t] for t in prompt]          # KeyError for an unknown token, like api_cache.py:162
    n_steps = int(max_len) - len(ids)
    if n_steps <= 0:
        toks = [id2tok[i] for i in ids]
        return (toks, [list(toks) for _ in range(n)], [float("-inf")] * n, 0) if return_all else toks
    if _no_window(eng) and len(ids) + n_steps > eng.max_ctx:
        raise RuntimeError(f"max_len={max_len} exceeds the engine's reserved context {eng.max_ctx}")
    eos = tok2id.get("[END_SEQUENCE]", -1)
    seed = _draw_seed() if seed is None else int(seed)
    gstate = None
    if grammar is not None:
        from .grammar import start_state
        _use_grammar(eng, grammar)
        gstate = start_state(grammar, ids)
    rows = [RowSampling(temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty, eos_id=eos,
                        seed=seed, stream=b, logit_bias=logit_bias, min_new_tokens=min(int(min_new_tokens), n_steps),
                        grammar_state=gstate, truncation=Truncation.of(min_p, typical_p, epsilon_cutoff, eta_cutoff))
            for b in range(n)]
    res = eng.generate_scored([ids] * n, rows, n_steps)
    out, lps = res.ids.cpu().tolist(), res.logprobs.cpu().tolist()
    best = pick_best(out, lps)
    cands = [[id2tok[t] for t in ids + [g for g in row if g >= 0]] for row in out]
    return (cands[best], cands, mean_logprobs(out, lps), best) if return_all else cands[best]


def _per_prompt(value, n: int, name: str) -> list:
    """a scalar for every prompt, or a list / tuple of exactly one value per prompt"""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} values for {n} prompts")
        return list(value)
    return [value] * n


def generate_requests(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                      top_p: Optional[float] = None, seed=None, repetition_penalty=None, logit_bias=None,
                      min_new_tokens=0, grammar=None,
                      min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, class_penalty=None) -> List[List[str]]:
    """Independent sample_kvcache requests served by one batched generation (up to the engine's max_batch rows per
    generation; more prompts take several).  Every argument may be a scalar or a list with one value per prompt.  Prompt i
    gets max_len_i - len(prompt_i) new tokens and stops after [END_SEQUENCE], like sample_kvcache; a seed of None is drawn
    with torch's generator (torch.manual_seed makes it reproducible).  Each row draws from Philox stream 0 under its own
    seed, the stream sample_kvcache uses for that seed.  Returns the prompt + generated tokens of each request, in order.
    Greedy rows (top_k=1) equal the reference run of their prompt alone; sampled rows depend on their own settings and on
    the batch size (kernel choice), not on the other requests.  logit_bias (one vector -- a dict, a host array or a device
    tensor [vocab] -- for every prompt, or a list with one per prompt, None = none) and min_new_tokens (capped at the prompt's
    budget) travel in the rows' records.  grammar (ONE TokenGrammar for all the prompts, or None) makes every row start in the state
    of its own prompt.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was.
    class_penalty (one mgea.decoder.ClassPenalty for every prompt, or a list with one per prompt, None = none): the row's windowed
    penalty over the classes of the engine's map (DecoderEngine.set_penalty_classes; generate_music.variety.token_classes)."""
    eng = _as_model(model)._need()
    ids = [[tok2id[t] for t in p] for p in prompts]   # KeyError for an unknown token, like api_cache.py:162
    budgets, live, rows = _request_rows(eng, ids, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias, min_new_tokens,
                                        grammar, min_p, typical_p, epsilon_cutoff, eta_cutoff, class_penalty, refuse_max_len=True)
    return _serve(eng, ids, budgets, live, lambda i: 1,
                  lambda part, steps: eng.generate_rows([ids[i] for i in part], [rows[i] for i in part], steps))


def _request_rows(eng, ids, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias, min_new_tokens, grammar,
                  min_p, typical_p, epsilon_cutoff, eta_cutoff, class_penalty=None, refuse_max_len=False):
    """The request table of the generate_requests* functions.  ids: each request's prompt -- its first variant -- as ids; every other
    argument a scalar for all the requests or a list with one value per request (grammar: ONE TokenGrammar or None).  Returns
    (budgets, live, rows): every request's max_len - len(prompt), the indices of those with a budget left, and {index: RowSampling}
    for them -- budget, seed (None = drawn here, in ascending order: a spent request draws none), Philox stream 0, min_new_tokens
    capped at the budget, the state its prompt leads to in the grammar, which becomes the engine's.
    refuse_max_len: a live request whose max_len exceeds the engine's context is refused here, before anything reaches the engine
    (generate_requests; the forms that cost more rows than one check prompt width + steps per generation, _check_fits)."""
    n = len(ids)
    max_lens = [int(v) for v in _per_prompt(max_len, n, "max_len")]
    temps = _per_prompt(temperature, n, "temperature")
    ks = _per_prompt(top_k, n, "top_k")
    ps = _per_prompt(top_p, n, "top_p")
    seeds = _per_prompt(seed, n, "seed")
    pens = _per_prompt(repetition_penalty, n, "repetition_penalty")
    biases = _per_prompt(logit_bias, n, "logit_bias")
    mins = [int(v) for v in _per_prompt(min_new_tokens, n, "min_new_tokens")]
    truncs = [Truncation.of(*v) for v in zip(_per_prompt(min_p, n, "min_p"), _per_prompt(typical_p, n, "typical_p"),
                                             _per_prompt(epsilon_cutoff, n, "epsilon_cutoff"), _per_prompt(eta_cutoff, n, "eta_cutoff"))]
    cpens = _per_prompt(class_penalty, n, "class_penalty")
    budgets = [L - len(p) for L, p in zip(max_lens, ids)]
    live = [i for i in range(n) if budgets[i] > 0]
    for i in live if refuse_max_len and _no_window(eng) else ():
        if max_lens[i] > eng.max_ctx:
            raise RuntimeError(f"max_len={max_lens[i]} exceeds the engine's reserved context {eng.max_ctx}")
    for i in range(n):
        if mins[i] < 0:
            raise ValueError(f"min_new_tokens: {mins[i]} for prompt {i} is negative")
    eos = tok2id.get("[END_SEQUENCE]", -1)
    gstates = [None] * n
    if grammar is not None:
        from .grammar import start_state
        _use_grammar(eng, grammar)
        gstates = [start_state(grammar, p) for p in ids]
    rows = {i: RowSampling(temperature=temps[i], top_k=ks[i], top_p=ps[i], repetition_penalty=pens[i], eos_id=eos,
                           max_new_tokens=budgets[i], seed=_draw_seed() if seeds[i] is None else int(seeds[i]), stream=0,
                           logit_bias=biases[i], min_new_tokens=min(mins[i], budgets[i]), grammar_state=gstates[i], truncation=truncs[i],
                           class_penalty=cpens[i])
            for i in live}
    return budgets, live, rows


def _serve(eng, ids, budgets, live, cost, run) -> List[List[str]]:
    """The serving loop of the generate_requests* functions: the live requests, in order, are cut into generations of as many whole
    requests as fit into the engine's max_batch rows -- cost(i): the rows request i takes -- and run(part, steps), the form's engine
    call for the requests `part` and their largest budget, returns their ids [len(part), steps].  Returns every request's prompt
    (ids[i]) + what it generated, as tokens; a request that is not live is its prompt."""
    gen: Dict[int, List[int]] = {}
    part, used = [], 0
    for i in live + [None]:   # (None: behind the last request)
        if part and (i is None or used + cost(i) > eng.max_batch):
            out = run(part, max(budgets[j] for j in part)).cpu().tolist()
            for j, row in zip(part, out):
                gen[j] = [g for g in row if g >= 0]
            part, used = [], 0
        if i is not None:
            part.append(i)
            used += cost(i)
    return [[id2tok[t] for t in ids[i] + gen.get(i, [])] for i in range(len(ids))]


def _check_fits(eng, width: int, steps: int) -> None:
    """A guided, scheduled or blended generation is never capped: without a KV window, prompt width + steps beyond the context is
    refused when its generation is reached."""
    if _no_window(eng) and width + steps > eng.max_ctx:
        raise RuntimeError(f"prompt width {width} + {steps} new tokens exceed the engine's reserved context {eng.max_ctx}")


def sample_kvcache_varied(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                          top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                          logit_bias=None, min_new_tokens: int = 0, grammar=None, classes="pitch", frequency_penalty: float = 0.0,
                          presence_penalty: float = 0.0, penalty_window: int = 32,
                          min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache_grammar with a windowed penalty over an ATTRIBUTE of the notes (sample_kvcache_grammar keeps its parameter
    list).  classes: which attribute -- "pitch", "pitch_class", "duration", "pitch_duration" or "id"
    (generate_music.variety.token_classes over the module's vocabulary) -- or a ready map, vocab ints with -1 = in no class.  With n_c
    the number of the last penalty_window generated tokens (0 = all of them, up to 4096 steps) of class c, every token of a class
    with n_c > 0 loses frequency_penalty * n_c + presence_penalty from its logit before the id-level repetition penalty, the bias,
    the grammar and the cuts; negative values keep the piece near the classes it has been using.  Both 0: the run that
    sample_kvcache_grammar makes.  The map becomes the engine's (DecoderEngine.set_penalty_classes) and stays set.  Build-defined:
    the reference has only the id-level repetition_penalty."""
    from mgea.decoder import ClassPenalty
    cp = ClassPenalty(frequency_penalty, presence_penalty, penalty_window)
    cp.check(0)
    if cp.on:
        _use_penalty_classes(_as_model(model)._need(), classes)
    return generate_requests(model, [prompt], max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias, min_new_tokens,
                             grammar, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff,
                             class_penalty=cp if cp.on else None)[0]


def _use_penalty_classes(eng, classes) -> None:
    """Make `classes` (a kind of variety.token_classes, or a ready map) the engine's penalty class map: uploaded when it is not
    what was set through here last."""
    import numpy as np
    from .variety import token_classes
    key = classes if isinstance(classes, str) else None
    m = token_classes(tok2id, classes) if key is not None else np.asarray(classes)
    if len(m) < eng.vocab:   # ids no token names are in no class
        m = np.concatenate([m, np.full(eng.vocab - len(m), -1, m.dtype)])
    last = getattr(eng, "_variety_classes", None)
    if last is not None and last[0] == key and np.array_equal(last[1], m) and eng.class_penalty_info()["n_class"] > 0:
        return
    eng.set_penalty_classes(m)
    eng._variety_classes = (key, m)


def sample_kvcache_guided(model, prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu",
                          top_p: Optional[float] = None, seed: Optional[int] = None, repetition_penalty: Optional[float] = None,
                          logit_bias=None, min_new_tokens: int = 0, grammar=None, guidance_scale: float = 1.5,
                          negative_prompt: Optional[Sequence[str]] = None,
                          min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache_grammar under classifier-free guidance (sample_kvcache_grammar keeps its parameter list): the request runs as a
    pair of rows, the prompt and negative_prompt -- None = the prompt without its [BPM] and [KEY_SIGNATURE] tokens
    (generate_music.guidance.unconditional_prompt) -- and every id is drawn from guidance_scale * logp(prompt) +
    (1 - guidance_scale) * logp(negative_prompt): 1 = the conditional distribution (not the same draws as sample_kvcache: a batch of
    two takes other kernels), above 1 the emotion tokens weigh more, 0 = the negative prompt alone.  Everything else -- penalty, bias,
    minimum length, grammar, the seed's Philox stream -- is the request's, applied to the mixed distribution.  Build-defined
    (DecoderEngine.generate_guided); the model needs max_batch >= 2.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    return generate_requests_guided(model, [prompt], max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias,
                                    min_new_tokens, grammar, guidance_scale,
                                    None if negative_prompt is None else [list(negative_prompt)],
                                    min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)[0]


def generate_requests_guided(model, prompts: Sequence[Sequence[str]], max_len=512, temperature=1.0, top_k=50,
                             top_p: Optional[float] = None, seed=None, repetition_penalty=None, logit_bias=None, min_new_tokens=0,
                             grammar=None, guidance_scale=1.5, negative_prompts=None,
                             min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[List[str]]:
    """generate_requests under classifier-free guidance: every request is a pair of rows (sample_kvcache_guided), so one generation
    serves up to max_batch // 2 of them.  guidance_scale: one value or one per prompt; negative_prompts: None = every prompt without
    its [BPM] / [KEY_SIGNATURE] tokens, else one token list per prompt (a None entry = that one's default).  Unlike generate_requests
    a request that would run past the engine's context is refused (RuntimeError) also where only its budget would be cut: a guided
    generation is never capped (a KV window lifts the limit).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    from .guidance import unconditional_prompt
    eng = _as_model(model)._need()
    n = len(prompts)
    scales = [float(v) for v in _per_prompt(guidance_scale, n, "guidance_scale")]
    negs = [None] * n if negative_prompts is None else list(negative_prompts)
    if len(negs) != n:
        raise ValueError(f"negative_prompts: {len(negs)} values for {n} prompts")
    negs = [unconditional_prompt(p) if q is None else list(q) for p, q in zip(prompts, negs)]
    ids = [[tok2id[t] for t in p] for p in prompts]   # KeyError for an unknown token, like api_cache.py:162
    neg_ids = [[tok2id[t] for t in q] for q in negs]
    if eng.max_batch < 2:
        raise ValueError("guided generation needs a model with max_batch >= 2 (a request is a pair of rows)")
    budgets, live, rows = _request_rows(eng, ids, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias, min_new_tokens,
                                        grammar, min_p, typical_p, epsilon_cutoff, eta_cutoff)

    def run(part, steps):
        _check_fits(eng, max(max(len(ids[i]), len(neg_ids[i])) for i in part), steps)
        return eng.generate_guided([ids[i] for i in part], [neg_ids[i] for i in part], [rows[i] for i in part],
                                   [scales[i] for i in part], steps)
    return _serve(eng, ids, budgets, live, lambda i: 2, run)


def sample_kvcache_transitions(model, prompts: Sequence[Sequence[str]], shares=None, max_len=512, temperature=1.0, top_k=50,
                               device="cpu", top_p: Optional[float] = None, seed: Optional[int] = None,
                               repetition_penalty: Optional[float] = None, logit_bias=None, min_new_tokens: int = 0, grammar=None,
                               guidance_scale: Optional[float] = None, negative_prompt: Optional[Sequence[str]] = None,
                               min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache_guided for a piece whose conditioning changes on the way (sample_kvcache_guided keeps its parameter list).
    prompts: 1 to 8 variants of ONE prompt, equal in length (generate_music.transitions.transition_prompts: the first with other
    [BPM] / [KEY_SIGNATURE] tokens); shares: the segments' relative lengths (None = equal).  The generation starts from prompts[0];
    when it enters segment s the cached keys and values of its prompt become those of prompts[s].  With a grammar
    (generate_music.grammar.track_grammar) the segments are ranges of note START classes (transitions.start_thresholds), so every
    track passes through all the emotions in musical time; without one they are ranges of steps (transitions.step_thresholds).
    guidance_scale None = no guidance; a number pairs the request with negative_prompt as sample_kvcache_guided does (the shadow row
    does not switch: it has no emotion tokens).  Returns prompts[0] + the generated tokens.  Build-defined
    (DecoderEngine.generate_scheduled).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    return generate_requests_transitions(model, [prompts], None if shares is None else [shares], max_len, temperature, top_k, top_p,
                                         seed, repetition_penalty, logit_bias, min_new_tokens, grammar, guidance_scale,
                                         None if negative_prompt is None else [list(negative_prompt)],
                                         min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)[0]


def generate_requests_transitions(model, prompt_segments: Sequence[Sequence[Sequence[str]]], shares=None, max_len=512,
                                  temperature=1.0, top_k=50, top_p: Optional[float] = None, seed=None, repetition_penalty=None,
                                  logit_bias=None, min_new_tokens=0, grammar=None, guidance_scale=None,
                                  negative_prompts=None,
                                  min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[List[str]]:
    """generate_requests_guided whose requests each bring the variants of their prompt (sample_kvcache_transitions) and, in shares, one
    list of relative segment lengths per request (None = equal).  guidance_scale None: no request is guided and a generation serves
    max_batch of them; otherwise every request is a pair and the limits of generate_requests_guided hold.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation); with none of them this is the call it always was."""
    from mgea.decoder import RowSchedule
    from .guidance import unconditional_prompt
    from .transitions import start_thresholds, step_thresholds
    eng = _as_model(model)._need()
    n = len(prompt_segments)
    segs = [[list(v) for v in ps] for ps in prompt_segments]
    for i, ps in enumerate(segs):
        if not ps or any(len(v) != len(ps[0]) for v in ps):
            raise ValueError(f"request {i}: the variants of a prompt must be of one length, got {[len(v) for v in ps]}")
    shares = [None] * n if shares is None else list(shares)
    if len(shares) != n:
        raise ValueError(f"shares: {len(shares)} values for {n} requests")
    guided = guidance_scale is not None
    scales = [float(v) for v in _per_prompt(guidance_scale if guided else 0.0, n, "guidance_scale")]
    negs = [None] * n if negative_prompts is None else list(negative_prompts)
    if len(negs) != n:
        raise ValueError(f"negative_prompts: {len(negs)} values for {n} requests")
    ids = [[[tok2id[t] for t in v] for v in ps] for ps in segs]   # KeyError for an unknown token, like api_cache.py:162
    neg_ids = [None] * n
    if guided:
        if eng.max_batch < 2:
            raise ValueError("guided generation needs a model with max_batch >= 2 (a request is a pair of rows)")
        neg_ids = [[tok2id[t] for t in (unconditional_prompt(ps[0]) if q is None else list(q))] for ps, q in zip(segs, negs)]
    first = [p[0] for p in ids]
    budgets, live, rows = _request_rows(eng, first, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias,
                                        min_new_tokens, grammar, min_p, typical_p, epsilon_cutoff, eta_cutoff)
    scheds = {}
    for i in live:
        sh = [1.0] * len(ids[i]) if shares[i] is None else list(shares[i])
        if len(sh) != len(ids[i]):
            raise ValueError(f"request {i}: {len(sh)} shares for {len(ids[i])} prompt variants")
        scheds[i] = RowSchedule(tuple(start_thresholds(grammar, sh)), 1) if grammar is not None else \
            RowSchedule(tuple(step_thresholds(budgets[i], sh)), 0)

    def run(part, steps):
        _check_fits(eng, max(max(len(first[i]), len(neg_ids[i] or [])) for i in part), steps)
        return eng.generate_scheduled([ids[i] for i in part], [rows[i] for i in part], [scheds[i] for i in part], steps,
                                      negative_prompts=[neg_ids[i] for i in part] if guided else None,
                                      guidance_scale=[scales[i] for i in part])
    return _serve(eng, first, budgets, live, lambda i: 2 if guided else 1, run)


def sample_kvcache_blended(model, prompts: Sequence[Sequence[str]], weights: Sequence[float], max_len=512, temperature=1.0, top_k=50,
                           top_p: Optional[float] = None, repetition_penalty: Optional[float] = None, device="cpu",
                           seed: Optional[int] = None, logit_bias=None, min_new_tokens: int = 0, grammar=None,
                           min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[str]:
    """sample_kvcache_grammar for one piece conditioned on several emotions at once.  prompts: 1 to 8 variants of ONE request
    (generate_music.blend.blend_prompts: the same instruments, another emotion's [BPM] / [KEY_SIGNATURE] tokens each, optionally the
    prompt without them as the last), weights: one finite weight per variant, summing to 1 (blend.blend_weights).  The request runs
    as a group of rows and every id is drawn from sum_k weights[k] * logp(prompts[k]), renormalised; everything else -- penalty (over
    prompts[0] and the generated ids), bias, minimum length, grammar, the seed's Philox stream -- is the request's, applied to the
    blended distribution.  Returns prompts[0] + the generated tokens.  Build-defined (DecoderEngine.generate_blended); the model needs
    max_batch >= len(prompts).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation)."""
    return generate_requests_blended(model, [prompts], [weights], max_len, temperature, top_k, top_p, repetition_penalty, seed, logit_bias,
                                     min_new_tokens, grammar, min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff,
                                     eta_cutoff=eta_cutoff)[0]


def generate_requests_blended(model, prompt_groups: Sequence[Sequence[Sequence[str]]], weights, max_len=512, temperature=1.0, top_k=50,
                              top_p: Optional[float] = None, repetition_penalty=None, seed=None, logit_bias=None, min_new_tokens=0,
                              grammar=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> List[List[str]]:
    """generate_requests whose requests each bring a group of prompt variants and one weight per variant (sample_kvcache_blended): a
    request of K variants is K rows, and one generation serves as many whole requests as fit into max_batch.  Every other argument is
    a scalar or a list with one value per request.  Like a guided request, a blended one that would run past the engine's context
    is refused (RuntimeError) also where only its budget would be cut: a blended generation is never capped (a KV window lifts the
    limit).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off; HuggingFace's names and semantics): further cuts behind top-k and top-p,
    in this order (mgea.decoder.Truncation)."""
    m = _as_model(model)
    eng = m._need()
    n = len(prompt_groups)
    groups = [[list(v) for v in g] for g in prompt_groups]
    weights = list(weights)
    if len(weights) != n:
        raise ValueError(f"weights: {len(weights)} lists for {n} requests")
    for i, g in enumerate(groups):
        if not g:
            raise ValueError(f"request {i}: no prompt")
        if len(weights[i]) != len(g):
            raise ValueError(f"request {i}: {len(weights[i])} weights for {len(g)} prompts")
        if len(g) > eng.max_batch:
            raise ValueError(f"request {i}: a group of {len(g)} rows needs a model with max_batch >= {len(g)}")
    ids = [[[tok2id[t] for t in v] for v in g] for g in groups]   # KeyError for an unknown token, like api_cache.py:162
    first = [g[0] for g in ids]
    budgets, live, rows = _request_rows(eng, first, max_len, temperature, top_k, top_p, seed, repetition_penalty, logit_bias,
                                        min_new_tokens, grammar, min_p, typical_p, epsilon_cutoff, eta_cutoff)

    def run(part, steps):
        _check_fits(eng, max(len(v) for i in part for v in ids[i]), steps)
        return eng.generate_blended([ids[i] for i in part], [list(weights[i]) for i in part], [rows[i] for i in part], steps)
    return _serve(eng, first, budgets, live, lambda i: len(ids[i]), run)


def sample(prompt: Sequence[str], max_len=512, temperature=1.0, top_k=50, device="cpu") -> List[str]:
    """generate_music/generate.py:46-61: same sampler over the module-level `model`.  With a
    GPTWithKV model this is sample_kvcache; with the post-LN twin `GPT` it recomputes the whole
    sequence every step exactly like the reference script (no cache is valid for that network)."""
    if model is None:
        raise RuntimeError("no module-level model: call load_checkpoint() or set generate.model")
    if not isinstance(model, GPT):
        return sample_kvcache(model, prompt, max_len, temperature, top_k, device)
    from mgea import ops
    ids = encode(prompt).unsqueeze(0)
    eos = tok2id.get("[END_SEQUENCE]", -1)
    for step in range(max_len - len(prompt)):
        logits = model(ids)[:, -1, :]
        nxt = ops.sample(logits, temperature, top_k, None, seed=_draw_seed(), step=step).cpu().long().view(1, 1)
        ids = torch.cat([ids, nxt], dim=1)
        if int(nxt) == eos:
            break
    return decode(ids.squeeze(0))
