"""bench.py's plain run on a small shape: the headline line only (no cpu_baseline, no extras, no roofline pass) and
--dump-outputs writing the ids of the last timed step, which must be the oracle's greedy ids for the bench's seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mgea import synth
from parity_util import check_greedy_vs_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    from mgea.decoder import DecoderEngine
    from oracle.decoder_ref import DecoderRef
    import bench as b

    B, Tp, TL = 4, 5, 96
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--total-len", str(TL),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-800:]
    line = json.loads(lines[0])
    assert line["metric"] == "midi_tokens_per_sec" and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - B * (TL - Tp) / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert line["roofline"] is None and "cpu_baseline" not in line and "extra" not in line

    assert sorted(os.listdir(tmp_path)) == ["generated_ids.npy"]
    ids = np.load(tmp_path / "generated_ids.npy")
    assert ids.dtype == np.float32 and ids.shape == (B, TL - Tp)
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 0 and ids.max() < b.DEC["vocab"]

    D = b.DEC
    sd = synth.decoder_state_dict(0, D["vocab"], D["seq_len"], D["d_model"], D["n_layer"])
    prompts = synth.integers(1, "prompts", (B, Tp), 0, D["vocab"]).tolist()
    eng = DecoderEngine(sd, n_head=b.N_HEAD, max_batch=B, max_ctx=TL, device="cuda:0")
    try:
        check_greedy_vs_oracle(eng, DecoderRef(sd, n_head=b.N_HEAD), prompts, TL - Tp, "bench --dump-outputs",
                               got=torch.from_numpy(ids.astype(np.int64)))
    finally:
        eng.close()
