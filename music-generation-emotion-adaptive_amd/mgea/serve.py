"""Request coalescing for the /generate endpoint: concurrent sample_kvcache requests served as one batched generation.

RequestBatcher owns one worker thread.  A request submitted while the worker is idle starts at once (no waiting window); requests
that arrive while a generation runs queue up, and the next generation takes up to `max_batch` of them -- one
generate_music.generate.generate_requests call, i.e. one mgea_decoder_generate_rows with each request's own settings, seed and
budget.  A short request still waits for the longest row of its batch (no admission into a running generation).
"""
from __future__ import annotations

import collections
import threading
from concurrent.futures import Future
from typing import List, Optional, Sequence


class _Request:
    __slots__ = ("tokens", "kwargs", "future", "grammar")

    def __init__(self, tokens, kwargs, future, grammar=None):
        self.tokens, self.kwargs, self.future, self.grammar = tokens, kwargs, future, grammar


class RequestBatcher:
    """Coalesces submit() calls from any number of threads into batched generations on `model` (a GPTWithKV).  The future of a
    request carries `batch_rows`, the number of requests its generation served, once it is done."""

    def __init__(self, model, max_batch: Optional[int] = None, autostart: bool = True):
        self.model = model
        self.max_batch = int(max_batch if max_batch is not None else model._need().max_batch)
        if self.max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self._queue = collections.deque()
        self._cv = threading.Condition()
        self._closed = False
        self._thread: Optional[threading.Thread] = None
        self._rows: List[int] = []
        if autostart:
            self.start()

    def start(self) -> None:
        with self._cv:
            if self._closed:
                raise RuntimeError("RequestBatcher is closed")
            if self._thread is None:
                self._thread = threading.Thread(target=self._worker, name="mgea-request-batcher", daemon=True)
                self._thread.start()

    def submit(self, prompt_tokens: Sequence[str], max_len=512, temperature=1.0, top_k=50, top_p=None,
               repetition_penalty=None, seed: Optional[int] = None, logit_bias=None, min_new_tokens: int = 0,
               grammar=None, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None,
               class_penalty=None) -> "Future[List[str]]":
        """Queue one sample_kvcache request; the future's result is its prompt + generated tokens.  Unknown tokens raise KeyError
        and a bad repetition penalty, logit_bias (a dict id -> bias, a host array or a device tensor [vocab]; a host one is checked
        in full, a device one for its shape) or min_new_tokens ValueError here, in the caller's thread.  A seed of None is drawn here too, so
        torch.manual_seed in the caller makes it reproducible whatever the batch it lands in.  grammar (a mgea.decoder.TokenGrammar or
        None, checked here): the engine holds one grammar at a time, so a batch serves requests that share the grammar object (or have
        none); a request with another one goes into the next batch.  min_p, typical_p, epsilon_cutoff, eta_cutoff (None = off;
        mgea.decoder.Truncation, checked here) travel in the request's own record, and so does class_penalty (a
        mgea.decoder.ClassPenalty or None, checked here; the class map is the engine's: DecoderEngine.set_penalty_classes)."""
        import generate_music.generate as gen
        from .ops import check_repetition_penalty
        tokens = list(prompt_tokens)
        for t in tokens:
            if t not in gen.tok2id:
                raise KeyError(t)
        check_repetition_penalty(repetition_penalty)
        if int(min_new_tokens) < 0:
            raise ValueError(f"min_new_tokens {min_new_tokens} is negative")
        if logit_bias is not None:
            from .decoder import check_logit_bias, dense_logit_bias
            eos = gen.tok2id.get("[END_SEQUENCE]", -1)
            logit_bias = dense_logit_bias(logit_bias, self.model._need().vocab)   # packed once, here, at the engine's vocabulary
            check_logit_bias(logit_bias, 0, eos, int(min_new_tokens), check=False)
        if grammar is not None:
            grammar.check(self.model._need().vocab)
        from .decoder import Truncation
        Truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff).check()
        if class_penalty is not None:
            class_penalty.check(0)
        kwargs = dict(max_len=int(max_len), temperature=temperature, top_k=top_k, top_p=top_p,
                      repetition_penalty=repetition_penalty, seed=gen._draw_seed() if seed is None else int(seed),
                      logit_bias=logit_bias, min_new_tokens=int(min_new_tokens), min_p=min_p, typical_p=typical_p,
                      epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, class_penalty=class_penalty)
        fut: Future = Future()
        with self._cv:
            if self._closed:
                raise RuntimeError("RequestBatcher is closed")
            self._queue.append(_Request(tokens, kwargs, fut, grammar))
            self._cv.notify()
        return fut

    def close(self) -> None:
        """Stop accepting requests, let the worker finish what is queued, and join it.  Requests of a batcher that was never
        started fail with RuntimeError."""
        with self._cv:
            self._closed = True
            self._cv.notify_all()
            thread = self._thread
        if thread is not None:
            thread.join()
        with self._cv:
            left = list(self._queue)
            self._queue.clear()
        for r in left:
            if r.future.set_running_or_notify_cancel():
                r.future.set_exception(RuntimeError("RequestBatcher closed before the request ran"))

    def stats(self) -> dict:
        """generations run so far and the number of requests each of them served"""
        with self._cv:
            return dict(generations=len(self._rows), rows_per_generation=list(self._rows), requests=sum(self._rows))

    # ------------------------------------------------------------------ worker
    def _worker(self) -> None:
        while True:
            with self._cv:
                while not self._queue and not self._closed:
                    self._cv.wait()
                if not self._queue:
                    return
                batch = [self._queue.popleft()]   # up to max_batch requests from the front, as long as they share the grammar object
                while self._queue and len(batch) < self.max_batch and self._queue[0].grammar is batch[0].grammar:
                    batch.append(self._queue.popleft())
            self._run(batch)

    def _run(self, batch: List[_Request]) -> None:
        import generate_music.generate as gen
        batch = [r for r in batch if r.future.set_running_or_notify_cancel()]
        if not batch:
            return
        kw = {k: [r.kwargs[k] for r in batch] for k in batch[0].kwargs}
        try:
            outs = gen.generate_requests(self.model, [r.tokens for r in batch], grammar=batch[0].grammar, **kw)
        except BaseException as e:   # this batch's requests fail; the worker serves the next one
            with self._cv:
                self._rows.append(len(batch))
            for r in batch:
                r.future.batch_rows = len(batch)
                r.future.set_exception(e)
            return
        with self._cv:
            self._rows.append(len(batch))
        for r, out in zip(batch, outs):
            r.future.batch_rows = len(batch)
            r.future.set_result(out)
