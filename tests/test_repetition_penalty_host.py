"""Repetition penalty, host side (no GPU): the fp32 restatement the GPU tests compare against, the presence-bitmap packer of
mgea.ops, argument checks and the public signatures."""
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def penalize(logits, seen, p):
    """transformers' RepetitionPenaltyLogitsProcessor restated in fp32: logits [B, V], seen = B iterables of ids (repeats
    allowed) or a bool [B, V] mask; for every seen id x -> x < 0 ? x * p : x / p with p held as fp32."""
    x = np.asarray(logits, dtype=np.float32)
    mask = np.zeros(x.shape, bool)
    if isinstance(seen, np.ndarray) and seen.dtype == bool:
        mask = seen
    else:
        for b, ids in enumerate(seen):
            mask[b, list(ids)] = True
    pf = np.float32(p)
    y = np.where(x < 0, x * pf, x / pf).astype(np.float32)
    return np.where(mask, y, x).astype(np.float32)


def test_restatement_matches_transformers_bitwise():
    tr = pytest.importorskip("transformers")
    rng = np.random.default_rng(5)
    B, V = 3, 700
    x = (rng.standard_normal((B, V)) * 6).astype(np.float32)
    x[:, :6] = [0.0, -0.0, 1e-40, -1e-40, 3.5, -3.5]          # +-0, denormals, exact values
    seen = [list(rng.integers(0, V, 250)) + [0, 1, 2, 3, 4, 5, 5, 5] for _ in range(B)]   # duplicates
    ids = torch.tensor(np.array(seen))
    for p in (1.1, 0.8, 1.5, 1.3, 2.0, 0.92):
        want = tr.RepetitionPenaltyLogitsProcessor(p)(ids, torch.from_numpy(x.copy())).numpy()
        got = penalize(x, seen, p)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), p


def test_pack_presence_matches_numpy_layout():
    from mgea import ops
    rng = np.random.default_rng(1)
    for V in (1, 31, 32, 33, 100, 8324, 14336):
        B = 3
        mask = rng.random((B, V)) < 0.3
        words = ops.pack_presence(mask, B, V)
        W = (V + 31) // 32
        assert words.shape == (B, W) and words.dtype == np.uint32
        want = np.zeros((B, W), np.uint32)
        for b, i in zip(*np.nonzero(mask)):
            want[b, i >> 5] |= np.uint32(1 << (i & 31))
        assert np.array_equal(words, want)
        assert np.array_equal(ops.pack_presence(torch.from_numpy(mask), B, V), want)
        lists = [list(np.nonzero(mask[b])[0]) * 2 for b in range(B)]   # repeated ids: same set
        assert np.array_equal(ops.pack_presence(lists, B, V), want)
        back = ops.unpack_presence(torch.from_numpy(words.view(np.int32)), V)
        assert np.array_equal(back.numpy(), mask)
    with pytest.raises(ValueError):
        ops.pack_presence([[100]], 1, 100)
    with pytest.raises(ValueError):
        ops.pack_presence(np.zeros((2, 5), bool), 1, 5)


@pytest.mark.parametrize("bad", [0.0, -1.1, float("nan"), float("inf"), -float("inf"), 1e-50, 1e300])
def test_bad_penalty_raises_value_error(bad):
    from mgea import ops
    with pytest.raises(ValueError):
        ops.check_repetition_penalty(bad)
    with pytest.raises(ValueError):   # before any device work: no GPU needed to see it
        ops.sample(torch.zeros(1, 4), repetition_penalty=bad)


def test_good_penalty_values():
    from mgea import ops
    assert ops.check_repetition_penalty(None) is None
    assert ops.check_repetition_penalty(1.1) == 1.1
    assert ops.check_repetition_penalty(1) == 1.0
    assert ops.check_repetition_penalty(0.5) == 0.5


def test_penalty_keyword_is_trailing_and_old_signatures_intact():
    import api_shim
    from generate_music import generate as gen
    from mgea import ops
    from mgea.decoder import DecoderEngine

    def params(f):
        return list(inspect.signature(f).parameters)

    assert params(gen.sample_kvcache) == ["model", "prompt", "max_len", "temperature", "top_k", "device", "top_p", "seed",
                                          "repetition_penalty"]
    assert params(gen.generate_sequence) == ["model_or_weights", "prompt", "max_len", "temperature", "top_k", "device", "top_p",
                                             "seed", "n_head", "repetition_penalty"]
    assert params(gen.generate_batch) == ["model", "prompts", "max_len", "temperature", "top_k", "top_p", "seed",
                                          "repetition_penalty"]
    assert params(DecoderEngine.generate) == ["self", "prompts", "n_steps", "temperature", "top_k", "top_p", "eos_id", "seed",
                                              "check_ids", "repetition_penalty"]
    assert params(ops.sample) == ["logits", "temperature", "top_k", "top_p", "seed", "step", "want_probs", "repetition_penalty",
                                  "presence"]
    assert params(api_shim.create_app) == ["model", "seq_len", "temperature", "top_k", "top_p", "repetition_penalty"]
    for f in (gen.sample_kvcache, gen.generate_sequence, gen.generate_batch, DecoderEngine.generate, ops.sample):
        assert inspect.signature(f).parameters["repetition_penalty"].default is None


def test_shim_rejects_bad_penalty_at_creation():
    import api_shim
    with pytest.raises(ValueError):
        api_shim.create_app(None, 64, repetition_penalty=-1.0)


def test_new_symbols_in_header_and_prototypes():
    from mgea import _lib
    with open(os.path.join(ROOT, "include", "mgea.h")) as f:
        hdr = f.read()
    for name in ("mgea_decoder_generate_penalized", "mgea_decoder_presence", "mgea_op_sample_penalized"):
        assert name + "(" in hdr, name
        assert name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["mgea_decoder_generate_penalized"][1][7] is _lib.C.c_float
    assert _lib.PROTOTYPES["mgea_op_sample_penalized"][1][4] is _lib.C.c_float
