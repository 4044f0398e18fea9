"""Request batching end to end ("Request batching"): concurrent clients against RequestBatcher versus one
sample_kvcache call per request.

Decoder-S (6L / 512d / V 8324) f32 synthetic weights, max_len 1024, top-k 50, ragged reference-shaped prompts (3 control tokens +
1..3 instruments).  For each client count, every client thread sends --requests requests back to back, either through
RequestBatcher.submit(...).result() (batched) or straight through sample_kvcache (one B = 1 generation per request, serialised
by the engine's lock -- what the endpoint does with batching off).  Prints one JSON line per (clients, mode): requests/s,
generated tokens/s, p50 / p95 request latency, and the batcher's rows per generation.

    python tools/serve_bench.py [--clients 1,8,32,64] [--requests 2] [--max-len 1024]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "music-generation-emotion-adaptive_amd"))

import torch  # noqa: E402

import generate_music.generate as gen  # noqa: E402
from mgea import synth  # noqa: E402
from mgea.serve import RequestBatcher  # noqa: E402


def run(clients, n_req, send):
    lat, toks = [], []
    lock = threading.Lock()

    def client(c):
        for r in range(n_req):
            t0 = time.perf_counter()
            out = send(c, r)
            dt = time.perf_counter() - t0
            with lock:
                lat.append(dt)
                toks.append(len(out))
    threads = [threading.Thread(target=client, args=(c,)) for c in range(clients)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    wall = time.perf_counter() - t0
    lat.sort()
    return dict(requests_per_s=round(len(lat) / wall, 3), tokens_per_s=round(sum(toks) / wall, 1),
                p50_ms=round(1e3 * statistics.median(lat), 1), p95_ms=round(1e3 * lat[min(len(lat) - 1, int(0.95 * len(lat)))], 1),
                wall_s=round(wall, 2), requests=len(lat))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", default="1,8,32,64")
    ap.add_argument("--requests", type=int, default=2, help="requests per client")
    ap.add_argument("--max-len", type=int, default=1024)
    a = ap.parse_args()
    V, L, C, NL, H = 8324, 1024, 512, 6, 8
    counts = [int(c) for c in a.clients.split(",")]
    sd = synth.decoder_state_dict(21, V, L, C, NL)
    gen.set_vocab(synth.decoder_vocab(V))   # no [END_SEQUENCE]: every request runs its whole budget
    model = gen.GPTWithKV(V, L, C, H, NL, max_batch=max(counts), max_ctx=L)
    model.load_state_dict(gen.remap_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}))
    bpm = [t for t in gen.tok2id if t.startswith("[BPM]")]
    keys = [t for t in gen.tok2id if t.startswith("[KEY_SIGNATURE]")]
    inst = [t for t in gen.tok2id if t.startswith("[INSTRUMENT]")]

    def prompt(c, r):   # api_cache.py:203: [START_SEQUENCE], BPM, key, 1..3 instruments
        return ["[START_SEQUENCE]", bpm[(c + r) % len(bpm)], keys[(3 * c + r) % len(keys)]] + inst[:1 + (c + r) % 3]

    plain = lambda c, r: gen.sample_kvcache(model, prompt(c, r), a.max_len, 1.0, top_k=50, seed=1000 * c + r)   # noqa: E731
    for n in counts:
        warm = RequestBatcher(model)   # capture the graphs of this batch size and of B = 1 first
        for f in [warm.submit(prompt(c, 0), a.max_len, top_k=50, seed=c) for c in range(n)]:
            f.result()
        warm.close()
        plain(0, 0)
        for mode in ("batched", "unbatched"):
            b = RequestBatcher(model) if mode == "batched" else None
            send = (lambda c, r: b.submit(prompt(c, r), a.max_len, top_k=50, seed=1000 * c + r).result()) if b else plain
            res = run(n, a.requests, send)
            if b:
                b.close()
                res["rows_per_generation"] = b.stats()["rows_per_generation"]
            print(json.dumps(dict(clients=n, mode=mode, max_len=a.max_len, **res)), flush=True)


if __name__ == "__main__":
    main()
