"""The reference's serving entry point on top of the MI355X hot path.

`create_app()` builds a FastAPI app whose `POST /generate` body follows api_cache.py:186-243 step by
step -- `inference.predict` -> `EATS.get_music_params` -> `closest_bpm_token` /
`normalize_key_signature` / `FAMILY_TO_INSTRUMENTS` -> `sample_kvcache` -> note tokens -> MIDI -- using
this repo's drop-in modules.  The only differences are the ones the offline box forces: the MIDI file
is written by generate_music.midi (pretty_midi absent) and returned directly as `audio/midi` instead
of being rendered to WAV by FluidSynth (midi2audio and the SoundFont are absent; rendering is outside
the accelerated path).
"""
from __future__ import annotations


CONSTRAINTS = (None, "notes", "scale")
GRAMMARS = (None, "tracks")


def create_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None):
    """top_p / repetition_penalty (None = none) reach sample_kvcache; the paper's decoding setting (§10.3) is
    create_app(model, seq_len, top_k=0, top_p=0.92, repetition_penalty=1.1).  One sample_kvcache call per request (they queue
    behind the engine's lock); create_batched_app serves concurrent requests as batches; create_constrained_app is this
    endpoint with a constraint on what may be drawn; create_windowed_app is it for pieces longer than the engine's context."""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False)


def create_windowed_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                        window=(1, None),
                        min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_app with a KV window (create_app keeps its parameter list; create_batched_app takes the same keyword).
    window = (sink_pages, ring_pages), ring_pages None = all the remaining pages: the model gets that window (GPTWithKV.set_window,
    max_steps = seq_len) and seq_len may exceed the engine's context -- a piece of more than max_ctx tokens, the prompt's
    conditioning tokens pinned in the sink while the oldest generated tokens leave (build-defined mechanics; the reference's loop
    has no context limit either, api_cache.py:159-184).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, window=window,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_constrained_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                           constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0):
    """create_app with a constraint on the tokens a request may draw (create_app keeps its parameter list; create_batched_app takes
    the same three options).
    constrain (build-defined, the reference samples the raw vocabulary): None = no constraint; "notes" = after the prompt only
    note, instrument and [END_SEQUENCE] tokens can be drawn (the detokeniser drops everything else); "scale" = also only notes of
    the emotion's key (mapping["key"]; out_of_scale_bias = -inf bans the others, a finite value is added to their logits instead).
    min_new_tokens > 0 keeps [END_SEQUENCE] from being drawn before that many tokens.  The bias vectors (generate_music.constraints)
    are built once per key and kept on the device; the response carries X-Constraint.  (create_grammar_app: this endpoint under a
    token grammar.)"""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens)


def create_grammar_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                       constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar="tracks",
                       min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_constrained_app under a token grammar (create_constrained_app keeps its parameter list; create_batched_app and
    create_best_of_app take the same keyword).  grammar (build-defined, the reference samples the raw vocabulary): None = none, or
    "tracks" = generate_music.grammar.track_grammar of the vocabulary -- after an instrument only a note may follow, a track's START
    times never go back, control tokens are not drawn.  Every request starts in the state its prompt leads to (OPEN: the prompt names
    the instruments); the response carries X-Grammar.  It composes with constrain="scale": the bias bans the out-of-scale notes, the
    grammar orders the rest.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_batched_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                       max_batch=None, grammar=None, window=None, constrain=None, out_of_scale_bias=float("-inf"),
                       min_new_tokens: int = 0):
    """create_app with request batching: concurrent requests are coalesced into batched generations by app.state.batcher
    (mgea.serve.RequestBatcher, up to max_batch rows each -- default the model's max_batch) instead of one sample_kvcache call per
    request.  Each request keeps its own seed and budget; the response also carries X-Batch-Rows, the number of requests its
    generation served.  app.state.batcher.close() stops the worker.  grammar: None or "tracks", as in create_grammar_app (the batcher
    groups requests by their grammar object; the app has one).  window: as in create_windowed_app (the requests' budgets are then not
    clamped at the engine's context)."""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=True, max_batch=max_batch,
                      constrain=constrain, out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar,
                      window=window)


def create_best_of_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                       best_of: int = 4, constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar=None,
                       min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_constrained_app whose requests draw best_of candidates in one batch and return the most likely one
    (generate_music.generate.generate_best_of: highest mean raw log-probability per generated token).  best_of is capped by the
    model's max_batch (ValueError here beyond it).  The response adds X-Best-Of and, when anything was generated, X-Mean-Logprob.  Build-defined: the reference
    draws one sequence per request.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    best_of = int(best_of)
    if best_of < 1 or best_of > int(model.max_batch):
        raise ValueError(f"best_of {best_of} outside [1, max_batch={model.max_batch}]")
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, best_of=best_of, grammar=grammar,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_guided_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                      constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar=None, guidance_scale: float = 1.5,
                      min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_grammar_app under classifier-free guidance (create_grammar_app keeps its parameter list; grammar defaults to None here).
    Every request runs as a pair of rows -- its prompt, and the prompt without the emotion's [BPM] and [KEY_SIGNATURE] tokens
    (generate_music.guidance.unconditional_prompt) -- and draws each id from guidance_scale * logp(prompt) + (1 - guidance_scale) *
    logp(the other): above 1 the piece follows the emotion's tempo and key more strongly than the model alone would, 1 is the
    conditional distribution, 0 ignores the emotion tokens (generate_music.generate.sample_kvcache_guided; build-defined, the
    reference has no guidance).  guidance_scale must be finite and >= 0 and the model needs max_batch >= 2 (ValueError here).  The
    response carries X-Guidance-Scale.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    import math
    guidance_scale = float(guidance_scale)
    if not (math.isfinite(guidance_scale) and guidance_scale >= 0):
        raise ValueError(f"guidance_scale {guidance_scale} must be finite and >= 0")
    if int(model.max_batch) < 2:
        raise ValueError(f"a guided request is a pair of rows: max_batch={model.max_batch} is too small")
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar, guidance_scale=guidance_scale,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_transition_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                          constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar="tracks",
                          guidance_scale=None,
                          min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_guided_app for a piece that follows the emotions of its text (create_guided_app keeps its parameter list; grammar
    defaults to "tracks" and guidance_scale to None = no guidance here).  The text goes through
    emotion_analysis.inference.analyze_emotion_transitions: one emotion, one EATS parameter set and one prompt variant per sentence
    (at most 8; generate_music.transitions.transition_prompts: the first sentence's prompt -- its instruments -- with each
    sentence's [BPM] and [KEY_SIGNATURE] tokens), the segments' shares the sentences' lengths.  Under the track grammar a segment is
    a range of note START classes, so every track walks through the emotions in musical time
    (generate_music.generate.sample_kvcache_transitions; build-defined, the reference labels the sentences and stops there); with
    grammar=None the segments are ranges of steps.  constrain="scale" keeps the FIRST sentence's key.  The response carries X-Emotions
    (the sentences' labels, comma-separated; X-Emotion is the first) and X-Segments.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    if guidance_scale is not None:
        import math
        guidance_scale = float(guidance_scale)
        if not (math.isfinite(guidance_scale) and guidance_scale >= 0):
            raise ValueError(f"guidance_scale {guidance_scale} must be finite and >= 0")
        if int(model.max_batch) < 2:
            raise ValueError(f"a guided request is a pair of rows: max_batch={model.max_batch} is too small")
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar, guidance_scale=guidance_scale,
                      transitions=True,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_truncated_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                         constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar=None,
                         min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, batch_requests: bool = False, max_batch=None,
                         window=None):
    """create_grammar_app (grammar defaults to None here) with HuggingFace's further truncation rules for every request: min_p,
    typical_p, epsilon_cutoff, eta_cutoff, None = off, applied in this order behind top-k and top-p inside the engine's sampler
    (mgea.decoder.Truncation; a value out of range is a ValueError here).  create_app, create_constrained_app and
    create_batched_app keep their parameter lists; every other create_*_app takes the same four keywords.  batch_requests=True
    serves concurrent requests as batches as create_batched_app does (max_batch, window: as there), each request with its record."""
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=bool(batch_requests),
                      max_batch=max_batch, constrain=constrain, out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens,
                      grammar=grammar, window=window,
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_blended_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                       constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar=None, top_emotions: int = 3,
                       min_prob: float = 0.05, guidance_scale=None,
                       min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_grammar_app for a piece conditioned on the text's emotion DISTRIBUTION, not on its arg-max alone (grammar defaults to
    None here).  The text goes through emotion_analysis.inference.predict_top_k_labels(text, top_emotions); the labels with a
    probability of at least min_prob are kept (the first always), each gives one EATS parameter set and one prompt -- the first
    label's instruments, that label's [BPM] and [KEY_SIGNATURE] tokens (generate_music.blend.blend_prompts) --, and the request runs
    as one group of rows that draws every id from sum_k w_k * logp(prompt k), w = the kept probabilities normalised
    (generate_music.generate.sample_kvcache_blended; build-defined, the reference has no consumer of its top-k labels).
    guidance_scale (None = none) adds the prompt without emotion tokens as one more member with weight 1 - guidance_scale and
    multiplies the others by guidance_scale.  constrain="scale" keeps the FIRST label's key.  top_emotions (+ 1 with a scale) must be
    in [1, 8] and fit into the model's max_batch (ValueError here).  The response carries X-Emotions (the kept labels,
    comma-separated; X-Emotion is the first) and X-Blend-Weights (the members' weights, comma-separated).
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    import math
    from generate_music.blend import MAX_ROWS
    top_emotions, min_prob = int(top_emotions), float(min_prob)
    if guidance_scale is not None:
        guidance_scale = float(guidance_scale)
        if not (math.isfinite(guidance_scale) and guidance_scale >= 0):
            raise ValueError(f"guidance_scale {guidance_scale} must be finite and >= 0")
    group = top_emotions + (guidance_scale is not None)
    if top_emotions < 1 or group > MAX_ROWS:
        raise ValueError(f"top_emotions {top_emotions}{'' if guidance_scale is None else ' + the unconditional prompt'} outside [1, {MAX_ROWS}] rows")
    if not (math.isfinite(min_prob) and 0 <= min_prob <= 1):
        raise ValueError(f"min_prob {min_prob} outside [0, 1]")
    if int(model.max_batch) < group:
        raise ValueError(f"a blended request is a group of up to {group} rows: max_batch={model.max_batch} is too small")
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar, guidance_scale=guidance_scale,
                      blend=(top_emotions, min_prob),
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def create_varied_app(model, seq_len: int, temperature: float = 1.0, top_k: int = 50, top_p=None, repetition_penalty=None,
                      constrain=None, out_of_scale_bias=float("-inf"), min_new_tokens: int = 0, grammar=None, classes="pitch",
                      frequency_penalty: float = 0.0, presence_penalty: float = 0.0, penalty_window: int = 32,
                      min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """create_grammar_app (grammar defaults to None here) with a windowed penalty over an attribute of the notes for every request
    (generate_music.generate.sample_kvcache_varied; build-defined, the reference has only the id-level repetition_penalty).
    classes: "pitch", "pitch_class", "duration", "pitch_duration" or "id" (generate_music.variety.token_classes); with n_c the number
    of the last penalty_window generated tokens (0 = all of them) of class c, every token of a class with n_c > 0 loses
    frequency_penalty * n_c + presence_penalty from its logit; negative values keep the piece near what it has been using.  A value
    that is not finite or beyond +-1e4, a window outside [0, 4096] and an unknown `classes` are ValueErrors here.  The response
    carries X-Penalty-Classes, X-Frequency-Penalty, X-Presence-Penalty and X-Penalty-Window.
    min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off): HuggingFace's further cuts behind top-k and top-p, for every request
    (mgea.decoder.Truncation; a value out of range is a ValueError here)."""
    from generate_music.variety import KINDS
    from mgea.decoder import ClassPenalty
    if classes not in KINDS:
        raise ValueError(f"classes must be one of {KINDS}, got {classes!r}")
    cp = ClassPenalty(float(frequency_penalty), float(presence_penalty), int(penalty_window))
    cp.check(0, max(int(seq_len), 0))
    return _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests=False, constrain=constrain,
                      out_of_scale_bias=out_of_scale_bias, min_new_tokens=min_new_tokens, grammar=grammar, variety=(classes, cp),
                      truncation=dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff))


def _build_app(model, seq_len, temperature, top_k, top_p, repetition_penalty, batch_requests, max_batch=None, constrain=None,
               out_of_scale_bias=float("-inf"), min_new_tokens=0, best_of=0, grammar=None, window=None, guidance_scale=None,
               transitions=False, truncation=None, blend=None, variety=None):
    from mgea.decoder import Truncation
    from mgea.ops import check_repetition_penalty
    check_repetition_penalty(repetition_penalty)   # a bad value fails here, not at the first request
    trunc_kw = {k: v for k, v in (truncation or {}).items() if v is not None}   # empty: every call below is what it was
    Truncation(**trunc_kw).check()
    if constrain not in CONSTRAINTS:
        raise ValueError(f"constrain must be one of {CONSTRAINTS}, got {constrain!r}")
    if grammar not in GRAMMARS:
        raise ValueError(f"grammar must be one of {GRAMMARS}, got {grammar!r}")
    out_of_scale_bias = float(out_of_scale_bias)
    if out_of_scale_bias != out_of_scale_bias or out_of_scale_bias == float("inf"):
        raise ValueError("out_of_scale_bias must be finite or -inf")
    if int(min_new_tokens) < 0:
        raise ValueError(f"min_new_tokens {min_new_tokens} is negative")
    if window is not None:   # (sink_pages, ring_pages); max_steps = what seq_len asks for
        sink_pages, ring_pages = window
        model.set_window(int(sink_pages), None if ring_pages is None else int(ring_pages), max_steps=max(int(seq_len), 1))
    from fastapi import FastAPI, Form
    from fastapi.middleware.cors import CORSMiddleware
    from fastapi.responses import Response

    import generate_music.generate as gen
    from emotion_analysis import EATS, inference
    from generate_music.midi import tokens_to_midi

    app = FastAPI()
    app.add_middleware(CORSMiddleware, allow_origins=["*"], allow_methods=["*"], allow_headers=["*"])
    try:   # the reference reads a multipart form field (api_cache.py:187); that needs python-multipart
        import multipart  # noqa: F401
        prompt_param = Form(...)
    except ImportError:   # absent on the offline box: same endpoint, `prompt` as a query parameter
        from fastapi import Query
        prompt_param = Query(...)
    app.state.prompt_in = "form" if prompt_param.__class__.__name__ == "Form" else "query"
    app.state.batcher = None
    app.state.on_tokens = None   # a callable set here receives every response's token list (tests look behind the MIDI with it)
    if batch_requests:
        from mgea.serve import RequestBatcher
        app.state.batcher = RequestBatcher(model, max_batch=max_batch)

    bias_cache = {}   # key token (None for "notes") -> the constraint's bias vector on the model's device

    def constraint_bias(key_token):
        if constrain is None:
            return None
        k = key_token if constrain == "scale" else None
        if k not in bias_cache:
            import torch
            from generate_music import constraints
            vec = constraints.logit_bias(gen.tok2id, key=k, notes_only=True, out_of_scale=out_of_scale_bias)
            bias_cache[k] = torch.from_numpy(vec).to(model._need().device)
        return bias_cache[k]

    grammar_cache = []   # the vocabulary's track grammar, built at the first request (ONE object: the batcher groups by it)

    def token_grammar():
        if grammar is None:
            return None
        if not grammar_cache:
            from generate_music.grammar import track_grammar
            grammar_cache.append(track_grammar(gen.tok2id))
        return grammar_cache[0]

    @app.post("/generate")
    def generate_music(prompt: str = prompt_param):
        sentences = []
        if transitions:   # one emotion per sentence; the first one's is the request's as far as the reference's steps go
            from generate_music.transitions import MAX_SEGMENTS
            sentences = inference.analyze_emotion_transitions(prompt)[:MAX_SEGMENTS]
        emotions = []
        if blend is not None:   # the text's most probable labels; those below min_prob go, the first never
            top = inference.predict_top_k_labels(prompt, blend[0])
            emotions = [top[0]] + [(lb, p) for lb, p in top[1:] if p >= blend[1]]
        label = emotions[0][0] if emotions else sentences[0][1] if sentences else inference.predict(prompt)   # api_cache.py:189
        mapping = EATS.get_music_params(label)                                # :190
        bpm_tok = gen.closest_bpm_token(mapping["bpm"])                       # :194
        key = gen.normalize_key_signature(mapping["key"])                     # :195
        instruments = []
        for fam in mapping["all_families"]:                                   # :196-198
            instruments.extend(gen.FAMILY_TO_INSTRUMENTS.get(fam, []))
        gen_prompt = ["[START_SEQUENCE]", bpm_tok, key] + [f"[INSTRUMENT] {i}" for i in instruments]   # :203
        extra = {}
        bias = constraint_bias(key)
        if constrain is not None:
            extra["X-Constraint"] = constrain
        more = {} if bias is None and not min_new_tokens else dict(logit_bias=bias, min_new_tokens=int(min_new_tokens))
        tg = token_grammar()
        if tg is not None:
            more["grammar"] = tg
            extra["X-Grammar"] = grammar
        if best_of:   # best_of candidates of the same request in one batch, the most likely one kept
            tokens, _, means, best = gen.generate_best_of(model, gen_prompt, best_of, max_len=seq_len, temperature=temperature,
                                                          top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                                                          logit_bias=bias, min_new_tokens=int(min_new_tokens), return_all=True,
                                                          grammar=tg, **trunc_kw)
            extra["X-Best-Of"] = str(best_of)
            if means[best] > float("-inf"):   # (nothing generated -- seq_len within the prompt -- has no mean)
                extra["X-Mean-Logprob"] = f"{means[best]:.6f}"
        elif blend is not None:   # one prompt per kept label, all of them one group of rows
            from generate_music.blend import blend_prompts, blend_weights
            # (the first label's parameters are the request's own: get_music_params may draw, and member 0 is gen_prompt itself)
            params = [mapping] + list(EATS.get_music_params([lb for lb, _ in emotions[1:]]))
            members = blend_prompts(gen_prompt, params, unconditional=guidance_scale is not None)
            weights = blend_weights([p for _, p in emotions], guidance_scale)
            tokens = gen.sample_kvcache_blended(model, members, weights, max_len=seq_len, temperature=temperature, top_k=top_k,
                                                top_p=top_p, repetition_penalty=repetition_penalty, device="cpu", logit_bias=bias,
                                                min_new_tokens=int(min_new_tokens), grammar=tg, **trunc_kw)
            extra["X-Emotions"] = ",".join(lb for lb, _ in emotions)
            extra["X-Blend-Weights"] = ",".join(f"{w:.4f}" for w in weights)
            if guidance_scale is not None:
                extra["X-Guidance-Scale"] = f"{guidance_scale:g}"
        elif transitions:   # one prompt variant per sentence, switched at the segments' boundaries
            from generate_music.transitions import transition_prompts
            sentences = sentences or [(prompt, label)]
            # (the first sentence's parameters are the request's own: get_music_params may draw, and variant 0 is gen_prompt itself)
            variants = transition_prompts(gen_prompt, [mapping] + [EATS.get_music_params(lb) for _, lb in sentences[1:]])
            tokens = gen.sample_kvcache_transitions(model, variants, [max(len(seg), 1) for seg, _ in sentences], max_len=seq_len,
                                                    temperature=temperature, top_k=top_k, device="cpu", top_p=top_p,
                                                    repetition_penalty=repetition_penalty, logit_bias=bias,
                                                    min_new_tokens=int(min_new_tokens), grammar=tg, guidance_scale=guidance_scale,
                                                    **trunc_kw)
            extra["X-Emotions"] = ",".join(lb for _, lb in sentences)
            extra["X-Segments"] = str(len(sentences))
            if guidance_scale is not None:
                extra["X-Guidance-Scale"] = f"{guidance_scale:g}"
        elif guidance_scale is not None:   # the request and its unconditional twin as one pair of rows
            tokens = gen.sample_kvcache_guided(model, gen_prompt, max_len=seq_len, temperature=temperature, top_k=top_k, device="cpu",
                                               top_p=top_p, repetition_penalty=repetition_penalty, logit_bias=bias,
                                               min_new_tokens=int(min_new_tokens), grammar=tg, guidance_scale=guidance_scale,
                                               **trunc_kw)
            extra["X-Guidance-Scale"] = f"{guidance_scale:g}"
        elif variety is not None:   # the request's own row, its logits lowered by the classes of its recent notes
            classes, cp = variety
            tokens = gen.sample_kvcache_varied(model, gen_prompt, max_len=seq_len, temperature=temperature, top_k=top_k, device="cpu",
                                               top_p=top_p, repetition_penalty=repetition_penalty, logit_bias=bias,
                                               min_new_tokens=int(min_new_tokens), grammar=tg, classes=classes,
                                               frequency_penalty=cp.frequency, presence_penalty=cp.presence,
                                               penalty_window=cp.window, **trunc_kw)
            extra["X-Penalty-Classes"] = classes
            extra["X-Frequency-Penalty"] = f"{cp.frequency:g}"
            extra["X-Presence-Penalty"] = f"{cp.presence:g}"
            extra["X-Penalty-Window"] = str(cp.window)
        elif app.state.batcher is not None:   # the same request, served inside whatever batch is forming
            fut = app.state.batcher.submit(gen_prompt, max_len=seq_len, temperature=temperature, top_k=top_k, top_p=top_p,
                                           repetition_penalty=repetition_penalty, **more, **trunc_kw)
            tokens = fut.result()
            extra["X-Batch-Rows"] = str(fut.batch_rows)
        else:
            call = gen.sample_kvcache_truncated if trunc_kw else gen.sample_kvcache_grammar if tg is not None else \
                gen.sample_kvcache_biased if more else gen.sample_kvcache
            tokens = call(model, gen_prompt, max_len=seq_len, temperature=temperature, top_k=top_k, device="cpu", top_p=top_p,
                          repetition_penalty=repetition_penalty, **more, **trunc_kw)   # :204
        if app.state.on_tokens is not None:
            app.state.on_tokens(tokens)
        midi = tokens_to_midi(tokens)                                         # :208-221 (+ pm.write)
        return Response(content=midi, media_type="audio/midi",
                        headers={"X-Emotion": label, "X-Prompt-Tokens": str(len(gen_prompt)),
                                 "X-Generated-Tokens": str(len(tokens)), **extra})

    return app
