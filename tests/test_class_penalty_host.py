"""Windowed penalties over token classes, host side (no device): the rule of include/mgea.h in numpy float32
(tests/class_penalty_util.py) and the premises the GPU tests rest on; what mgea.decoder.ClassPenalty refuses, naming the row; the
packing and the inheritance of the records; generate_music.variety.token_classes; the C ABI's declarations and the surface; the plan
of a class-penalised generation (tests/native/class_penalty_plan_test.cpp, a stand-alone host program over csrc/gen_plan.h)."""
import ctypes as C
import dataclasses
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from class_penalty_util import counts, host_rule
from mgea import synth
from mgea.decoder import CLASS_PENALTY_MAX_WINDOW, ClassPenalty, RowSampling, Truncation, pack_blended, pack_class_penalty, pack_guided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_window_edges():
    class_of = np.array([0, 1, 2, -1, 0, 1], np.int32)
    hist = np.array([[0, 1, 2, 3, 4, 5, 2, 2]], np.int32)          # classes 0 1 2 - 0 1 2 2
    for t, w, want in ((8, 0, [2, 2, 3]), (8, 8, [2, 2, 3]), (8, 9, [2, 2, 3]), (8, 7, [1, 2, 3]), (8, 2, [0, 0, 2]), (8, 1, [0, 0, 1]),
                       (4, 0, [1, 1, 1]), (4, 3, [0, 1, 1]), (4, 1, [0, 0, 0]), (1, 5, [1, 0, 0]), (0, 0, [0, 0, 0]), (0, 3, [0, 0, 0])):
        assert counts(hist[0], t, w, class_of, 3).tolist() == want, (t, w)
    x = np.arange(12, dtype=np.float32).reshape(2, 6)
    got = host_rule(x, class_of, hist, [8], [0], [(0.5, 2.0, 2)])                 # n = [0, 0, 2]: class 2 alone, d = 0.5 * 2 + 2 = 3
    assert got[0].tolist() == [0, 1, 2 - 3, 3, 4, 5] and got[1].tobytes() == x[1].tobytes(), "only id 2 of row 0 is written"
    # entries outside [0, vocab) are skipped, never indexed
    bad = np.array([[7, -1, 2, 99]], np.int32)
    assert counts(bad[0], 4, 0, class_of, 3).tolist() == [0, 0, 1]


def test_what_is_not_written_comes_back_bit_for_bit():
    rng = np.random.default_rng(3)
    V = 40
    class_of = (np.arange(V) % 5).astype(np.int32)
    class_of[::7] = -1
    x = rng.standard_normal((6, V)).astype(np.float32)
    x[0, 3] = -0.0                                                   # (a sign a "- 0" would lose)
    hist = rng.integers(0, V, (5, 16)).astype(np.int32)
    hist[4, :] = 1                                                   # row 4 counts class 1 alone
    recs = [(0.0, 0.0, 4), (0.5, 1.0, 4), (0.5, 1.0, 4), (-0.0, 0.0, 0), (0.25, 0.0, 0)]
    got = host_rule(x, class_of, hist, [9, 9, 0, 9, 9], [0, 1, 0, 0, 0], recs)
    for b, why in ((0, "off"), (1, "finished"), (2, "t == 0"), (3, "off (-0)"), (5, "behind the batch")):
        assert got[b].tobytes() == x[b].tobytes(), why
    hit = class_of == 1
    assert np.array_equal(got[4, ~hit], x[4, ~hit]) and got[4, ~hit].tobytes() == x[4, ~hit].tobytes(), "class -1 and uncounted classes"
    assert np.array_equal(got[4, hit], x[4, hit] - np.float32(0.25 * 9))
    # done == 2 (a parked row) is finished too
    assert host_rule(x, class_of, hist, [9] * 5, [2] * 5, recs).tobytes() == x.tobytes()


def test_counts_up_to_4096_are_exact_in_fp32_and_the_three_roundings_are_separate():
    n = np.arange(1, CLASS_PENALTY_MAX_WINDOW + 1)
    assert np.array_equal(n.astype(np.float32).astype(np.int64), n), "every count up to 4096 is a float32"
    # the rule rounds f * n, then + p, then x - d; one fused multiply-add rounds f * n + p once and differs in the last bit somewhere
    f, p = np.float32(-0.7), np.float32(2.5)
    two = (f * n.astype(np.float32)).astype(np.float32) + p
    one = (np.float64(f) * n + np.float64(p)).astype(np.float32)       # exact product and sum (53 bits hold both), rounded once
    assert two.dtype == np.float32 and int((two != one).sum()) > 0, "the fused form would be indistinguishable: the GPU test would show nothing"
    V = 8
    class_of = np.zeros(V, np.int32)
    hist = np.zeros((1, CLASS_PENALTY_MAX_WINDOW), np.int32)
    x = np.full((1, V), 0.1, np.float32)
    for t in (1, 3, 255, 4095, 4096):
        got = host_rule(x, class_of, hist, [t], [0], [(float(f), float(p), 0)])
        m = np.float32(f * np.float32(t))
        assert got[0, 0] == np.float32(np.float32(0.1) - np.float32(m + p)), t
    # negative values favour the counted classes
    assert (host_rule(x, class_of, hist, [4], [0], [(-1.0, -1.0, 0)]) > x).all()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_class_penalty_check_names_the_row():
    assert not ClassPenalty().on and not ClassPenalty(0.0, -0.0, 9).on and ClassPenalty(0, 1e-30).on and ClassPenalty(-1).on
    assert not ClassPenalty(1e-60, 0).on, "a value that is 0 as the float32 the record holds is off"
    for ok in (ClassPenalty(1e4, -1e4, 4096), ClassPenalty(0, 0, 0), ClassPenalty(0.5, 2.0, 4)):
        ok.check(3, 4096, 12)
    for bad in (math.nan, math.inf, -math.inf, 1.0001e4, -2e4, 1e39):
        with pytest.raises(ValueError, match="row 2: frequency .* finite and within"):
            ClassPenalty(bad, 0, 4).check(2)
        with pytest.raises(ValueError, match="row 5: presence .* finite and within"):
            ClassPenalty(0, bad, 4).check(5)
    for w in (-1, 4097, 2.5):
        with pytest.raises(ValueError, match=r"row 1: window .* outside \[0, 4096\]"):
            ClassPenalty(0.5, 0, w).check(1)
        with pytest.raises(ValueError, match="row 1: window"):
            ClassPenalty(0, 0, w).check(1)                       # a record that is off is checked too
    with pytest.raises(ValueError, match="row 4: window 0 .* 4097 steps"):
        ClassPenalty(0.5, 0, 0).check(4, 4097)
    ClassPenalty(0.5, 0, 0).check(4, 4096)
    ClassPenalty(0.0, 0, 0).check(4, 4097)
    with pytest.raises(ValueError, match="row 0 has a class penalty but no class map"):
        ClassPenalty(0.5, 0, 4).check(0, 10, 0)
    ClassPenalty(0.0, 0, 4).check(0, 10, 0)
    rec = ClassPenalty(0.5, -2.0, 7).record()
    assert (rec.frequency, rec.presence, rec.window, rec.reserved) == (0.5, -2.0, 7, 0)
    with pytest.raises(ValueError, match="row 1: class_penalty must be a ClassPenalty"):
        RowSampling(class_penalty=(0.5, 0, 4)).check(1, 100)
    with pytest.raises(ValueError, match="row 1: presence"):
        RowSampling(class_penalty=ClassPenalty(0, math.nan)).check(1, 100)


def test_row_sampling_carries_the_record_like_truncation():
    assert [f.name for f in dataclasses.fields(RowSampling)] == ["temperature", "top_k", "top_p", "repetition_penalty", "eos_id",
                                                                 "max_new_tokens", "seed", "stream", "logit_bias", "min_new_tokens"]
    cp = ClassPenalty(0.5, 1.0, 8)
    r = RowSampling(1.0, 20, seed=4, truncation=Truncation(min_p=0.1), class_penalty=cp)
    assert r.class_penalty is cp and RowSampling().class_penalty is None
    r2 = dataclasses.replace(r, seed=5)
    assert r2.class_penalty is cp and r2.truncation is r.truncation and r2.seed == 5
    assert dataclasses.replace(r, class_penalty=None).class_penalty is None
    assert list(inspect.signature(RowSampling).parameters)[-3:] == ["grammar_state", "truncation", "class_penalty"]


def test_packing():
    on, off = ClassPenalty(0.5, 1.0, 8), ClassPenalty(0, 0, 3)
    assert pack_class_penalty([RowSampling(), RowSampling()]) is None
    assert pack_class_penalty([RowSampling(class_penalty=off), RowSampling()]) is None, "records that are all off: the call there always was"
    recs = pack_class_penalty([RowSampling(), RowSampling(class_penalty=on), RowSampling(class_penalty=off)], 100, 12)
    assert len(recs) == 3 and [(r.frequency, r.presence, r.window, r.reserved) for r in recs] == [(0, 0, 0, 0), (0.5, 1.0, 8, 0), (0, 0, 3, 0)]
    with pytest.raises(ValueError, match="row 1: frequency"):
        pack_class_penalty([RowSampling(), RowSampling(class_penalty=ClassPenalty(math.inf))])
    with pytest.raises(ValueError, match="row 1 has a class penalty but no class map"):
        pack_class_penalty([RowSampling(), RowSampling(class_penalty=on)], 100, 0)
    with pytest.raises(ValueError, match="row 0: window 0"):
        pack_class_penalty([RowSampling(class_penalty=ClassPenalty(1.0))], 5000, 12)


def test_shadow_rows_and_members_inherit_the_record():
    a, b = ClassPenalty(0.5, 1.0, 8), ClassPenalty(0, 1e4, 4)
    rows = [RowSampling(seed=1, class_penalty=a), RowSampling(seed=2), RowSampling(seed=3, class_penalty=b)]
    prompts, all_rows, shadow, _, _ = pack_guided([[1, 2], [3], [4, 5]], [[1], None, [4]], rows, 1.5, 8)
    assert shadow[:3] == [3, -1, 4] and len(all_rows) == 5
    assert all_rows[3].class_penalty is a and all_rows[4].class_penalty is b, "a shadow row carries its conditional row's record"
    recs = pack_class_penalty(all_rows, 16, 12)
    assert [(r.frequency, r.presence, r.window) for r in recs] == [(0.5, 1.0, 8), (0, 0, 0), (0, 1e4, 4), (0.5, 1.0, 8), (0, 1e4, 4)]
    _, all_rows, leader, _, _ = pack_blended([[[1], [2], [3]], [[4]], [[5], [6]]], [[0.6, 0.3, 0.1], [1.0], [0.5, 0.5]], rows, 8)
    assert leader == [0, -1, 2, 0, 0, 2]
    for u, l in enumerate(leader):
        if l >= 0:
            assert all_rows[u].class_penalty is all_rows[l].class_penalty, "a member carries its leader's record"
    assert all_rows[1].class_penalty is None


# ------------------------------------------------------------------------------------------------------------ token_classes
def test_token_classes_on_a_synthetic_vocabulary():
    from generate_music.midi import note_name_to_number, note_re
    from generate_music.variety import KINDS, token_classes
    tok2id = synth.decoder_vocab(200, with_eos=True)
    notes = {i: note_re.match(t) for t, i in tok2id.items() if t.startswith("[NOTE]")}
    assert len(notes) == 200 - 36 and KINDS == ("pitch", "pitch_class", "duration", "pitch_duration", "id")
    for by in KINDS:
        m = token_classes(tok2id, by)
        assert m.dtype == np.int32 and m.shape == (200,)
        assert all(m[i] == -1 for t, i in tok2id.items() if not t.startswith("[NOTE]")), "every non-note token is in no class"
        assert all(m[i] >= 0 for i in notes) and sorted(set(m[m >= 0].tolist())) == list(range(int(m.max()) + 1)), "dense classes"
    pitch = {i: note_name_to_number(mt.group(1)) for i, mt in notes.items()}
    dur = {i: float(mt.group(4)) for i, mt in notes.items()}
    for by, key in (("pitch", pitch), ("pitch_class", {i: p % 12 for i, p in pitch.items()}), ("duration", dur),
                    ("pitch_duration", {i: (pitch[i], dur[i]) for i in notes}), ("id", {i: i for i in notes})):
        m = token_classes(tok2id, by)
        ids = sorted(notes)
        for i in ids[:40]:
            for j in ids[:40]:
                assert (m[i] == m[j]) == (key[i] == key[j]) and (m[i] < m[j]) == (key[i] < key[j]), (by, i, j)
    assert token_classes(tok2id, "pitch_class").max() == 11 and token_classes(tok2id, "duration").max() == 2
    assert token_classes(tok2id, "id").max() == len(notes) - 1
    # enharmonic spellings are one pitch
    two = {"[NOTE] [PITCH:C#4] [START:0.0] [END:1.0] [DURATION:1.0]": 0, "[NOTE] [PITCH:D-4] [START:0.5] [END:1.0] [DURATION:0.5]": 1,
           "[PAD]": 3}
    assert token_classes(two, "pitch").tolist() == [0, 0, -1, -1] and token_classes(two, "duration").tolist() == [1, 0, -1, -1]
    with pytest.raises(ValueError, match="by = 'timbre'"):
        token_classes(tok2id, "timbre")
    with pytest.raises(ValueError, match="no note"):
        token_classes({"[PAD]": 0}, "pitch")


# ------------------------------------------------------------------------------------------------ the C ABI and the surface
def test_the_c_abi_declares_the_class_penalty_entry_points():
    from mgea import _lib
    hdr = open(os.path.join(ROOT, "include", "mgea.h")).read()
    lib = _lib.load()
    for name in ("mgea_decoder_set_penalty_classes", "mgea_decoder_generate_rows_class_penalized", "mgea_decoder_class_penalty_info",
                 "mgea_op_class_penalty"):
        assert name + "(" in hdr and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "#define MGEA_CLASS_PENALTY_MAX_WINDOW 4096" in hdr and _lib.CLASS_PENALTY_MAX_WINDOW == 4096
    assert C.sizeof(_lib.RowClassPenalty) == 16
    assert [f[0] for f in _lib.RowClassPenalty._fields_] == ["frequency", "presence", "window", "reserved"]
    blend, cpen = (_lib.PROTOTYPES[f"mgea_decoder_generate_rows_{n}"][1] for n in ("blended", "class_penalized"))
    assert cpen[:len(blend) - 1] == blend[:-1] and cpen[-2:] == [C.POINTER(_lib.RowClassPenalty), C.c_void_p]


def test_surface():
    import api_shim
    import generate_music.generate as gen
    from mgea import ops
    from mgea.decoder import DecoderEngine
    from mgea.serve import RequestBatcher
    sig = inspect.signature(gen.sample_kvcache_varied).parameters
    assert list(sig)[:3] == ["model", "prompt", "max_len"]
    assert (sig["classes"].default, sig["frequency_penalty"].default, sig["presence_penalty"].default, sig["penalty_window"].default) == \
        ("pitch", 0.0, 0.0, 32)
    sig = inspect.signature(api_shim.create_varied_app).parameters
    assert (sig["classes"].default, sig["frequency_penalty"].default, sig["presence_penalty"].default, sig["penalty_window"].default) == \
        ("pitch", 0.0, 0.0, 32)
    assert inspect.signature(gen.generate_requests).parameters["class_penalty"].default is None
    assert inspect.signature(RequestBatcher.submit).parameters["class_penalty"].default is None
    assert list(inspect.signature(ops.class_penalty).parameters) == ["logits", "class_of", "hist", "row_step", "done", "recs"]
    assert callable(DecoderEngine.set_penalty_classes) and callable(DecoderEngine.class_penalty_info)

    class Model:
        max_batch = 2
    with pytest.raises(ValueError, match="classes must be one of"):
        api_shim.create_varied_app(Model(), 64, classes="timbre")
    with pytest.raises(ValueError, match="row 0: frequency"):
        api_shim.create_varied_app(Model(), 64, frequency_penalty=math.nan)
    with pytest.raises(ValueError, match="row 0: window"):
        api_shim.create_varied_app(Model(), 64, presence_penalty=1.0, penalty_window=-3)
    with pytest.raises(ValueError, match="row 0: window 0"):
        api_shim.create_varied_app(Model(), 5000, presence_penalty=1.0, penalty_window=0)


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_class_penalty_plan_native(tmp_path):
    """tests/native/class_penalty_plan_test.cpp: kind.class_penalized, never GREEDY, next to every other flag, every refusal, NULL /
    all-off records => the blended plan.  A stand-alone host program; with AddressSanitizer and UBSan where there is no GPU."""
    exe = str(tmp_path / "class_penalty_plan_test")
    san = [] if torch.cuda.is_available() else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *san,
                           os.path.join(ROOT, "tests", "native", "class_penalty_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "class_penalty_plan ok" and r.stderr == "", r.stdout + r.stderr
