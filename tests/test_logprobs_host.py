"""Host side of the log-probability work: pick_best / mean_logprobs, the packing of forced ids and its ValueErrors, the best-of cap,
and the new C-ABI symbols.  No GPU needed."""
import math

import numpy as np
import pytest
import torch

from mgea import _lib
from mgea.decoder import pack_force_ids

NINF = -math.inf


def test_pick_best_means_are_over_produced_ids_only():
    from generate_music.generate import mean_logprobs, pick_best
    ids = [[5, 6, -1, -1], [7, 8, 9, 10], [3, -1, -1, -1]]
    lps = [[-1.0, -3.0, 0.0, 0.0], [-2.0, -2.0, -2.0, -4.0], [-2.25, 0.0, 0.0, 0.0]]
    # row 0: (-1 - 3) / 2 = -2 (the zeros behind its EOS do not dilute it to -1), row 1: -2.5, row 2: -2.25
    assert mean_logprobs(ids, lps) == [-2.0, -2.5, -2.25]
    assert pick_best(ids, lps) == 0
    assert pick_best(np.asarray(ids), np.asarray(lps)) == 0
    # values written behind a finish are ignored even if they are not zero
    assert mean_logprobs([[5, -1]], [[-1.5, -100.0]]) == [-1.5]


def test_pick_best_ties_go_to_the_lowest_index():
    from generate_music.generate import pick_best
    ids = [[1, 2], [3, 4], [5, 6]]
    assert pick_best(ids, [[-2.0, -2.0], [-1.0, -1.0], [-0.5, -1.5]]) == 1
    assert pick_best(ids, [[-1.0, -1.0], [-1.0, -1.0], [-1.0, -1.0]]) == 0


def test_pick_best_row_without_ids_scores_minus_inf():
    from generate_music.generate import mean_logprobs, pick_best
    ids = [[-1, -1], [4, -1], [-1, -1]]
    lps = [[0.0, 0.0], [-50.0, 0.0], [0.0, 0.0]]
    assert mean_logprobs(ids, lps) == [NINF, -50.0, NINF]
    assert pick_best(ids, lps) == 1
    assert pick_best([[-1], [-1]], [[0.0], [0.0]]) == 0   # nothing produced anywhere: still the lowest index


def test_force_ids_packing():
    assert pack_force_ids(None, 2, 4, 10) is None
    got = pack_force_ids([[1, 2], [], [3, -1, 9]], 3, 4, 10)
    assert got.dtype == torch.int32 and got.tolist() == [[1, 2, -1, -1], [-1, -1, -1, -1], [3, -1, 9, -1]]
    assert pack_force_ids([None, (4,)], 2, 2, 10).tolist() == [[-1, -1], [4, -1]]
    t = pack_force_ids(torch.tensor([[0, 9], [-1, 3]]), 2, 3, 10)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 9, -1], [-1, 3, -1]]
    full = torch.tensor([[0, 1, 2]], dtype=torch.int64)
    assert pack_force_ids(full, 1, 3, 10).tolist() == [[0, 1, 2]]


def test_force_ids_value_errors_name_the_row():
    with pytest.raises(ValueError, match="row 1"):
        pack_force_ids([[1], [10]], 2, 4, 10)             # == vocab
    with pytest.raises(ValueError, match="row 0"):
        pack_force_ids([[-2], [1]], 2, 4, 10)             # below -1
    with pytest.raises(ValueError, match="row 2"):
        pack_force_ids(torch.tensor([[0], [1], [77]]), 3, 4, 10)
    with pytest.raises(ValueError, match="row 1"):
        pack_force_ids([[1], [1, 2, 3]], 2, 2, 10)        # more ids than steps
    with pytest.raises(ValueError):
        pack_force_ids([[1]], 2, 4, 10)                   # one row for two prompts
    with pytest.raises(ValueError):
        pack_force_ids(torch.zeros(2, 5, dtype=torch.int64), 2, 4, 10)   # wider than the steps
    with pytest.raises(ValueError):
        pack_force_ids(torch.zeros(2, 3), 2, 4, 10)       # not an int tensor


def test_best_of_is_capped_by_max_batch():
    import generate_music.generate as gen
    from api_shim import create_best_of_app
    model = gen.GPTWithKV(100, 16, 32, 2, 1, max_batch=4)   # no weights: the cap is checked before the engine is needed
    with pytest.raises(ValueError, match="max_batch"):
        gen.generate_best_of(model, ["a"], 5)
    with pytest.raises(ValueError):
        gen.generate_best_of(model, ["a"], 0)
    with pytest.raises(RuntimeError):                       # n within the cap reaches the (missing) engine
        gen.generate_best_of(model, ["a"], 4)
    with pytest.raises(ValueError, match="max_batch"):
        create_best_of_app(model, 16, best_of=5)


def test_new_symbols_are_bound():
    for name in ("mgea_decoder_generate_rows_scored", "mgea_op_sample_rows_scored"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
    assert len(_lib.PROTOTYPES["mgea_decoder_generate_rows_scored"][1]) == 13
    assert len(_lib.PROTOTYPES["mgea_op_sample_rows_scored"][1]) == 13


def test_fp32_formula_error_at_the_test_sizes():
    """The formula's own fp32 rounding: x_id - m - log(sum exp(x_i - m)) with numpy's fp32 exp and sequential partial sums stays
    within 2e-6 of float64 on N(0, 3) rows of the sizes used on the GPU.  This says nothing about the kernel's arithmetic (__expf, a
    butterfly reduction): that is bounded only by the 1e-4 of tests/test_gpu_logprobs.py, which this figure shows to be wide enough
    for fp32."""
    rng = np.random.default_rng(3)
    for V in (100, 8324, 14336):
        x = (rng.standard_normal((4, V)) * 3).astype(np.float32)
        m = x.max(1, keepdims=True)
        s = np.zeros(4, np.float32)
        for c in range(0, V, 256):   # sequential fp32 partial sums, thread-like order
            s += np.exp(x[:, c:c + 256] - m, dtype=np.float32).sum(1, dtype=np.float32)
        got = x - m - np.log(s, dtype=np.float32)[:, None]
        want = torch.log_softmax(torch.from_numpy(x).double(), dim=1).numpy()
        err = float(np.abs(got - want).max())
        print(f"[logprobs] V={V}: fp32 formula vs float64 {err:.2e}")
        assert err < 2e-6
