"""CPU checks of what the causal-mode GPU tests stand on (tests/causal_util.py): the input families against fp64 at every shape the GPU
tests use, CausalRef against the golden-pinned oracle and against itself, the host rules of a causal generation's prefill, and the oracle of the
generation forms (causal_step_logits, walk) with the input conditions of every case test_gpu_causal_forms.py runs."""
import numpy as np
import pytest
import torch

import causal_util as U
from mgea import synth
from oracle.decoder_ref import DecoderRef


@pytest.mark.parametrize("dh", U.DENSE_DH)
@pytest.mark.parametrize("kind", ["none", "ragged"])
def test_dense_families_equal_fp64_causal_attention(kind, dh):
    """CausalCase asserts the closed form against fp64 (1e-6) and fp16 exactness when it is built"""
    for T in U.DENSE_T:
        for family in U.FAMILIES:
            c = U.dense_case(family, kind, T, dh)
            assert c.rows.any()
            if kind == "ragged":
                assert not c.rows[1].any() and c.rows[2].sum() == 1       # the rows of length 0 and 1


@pytest.mark.parametrize("dh", U.PAGED_DH)
@pytest.mark.parametrize("ctx", U.PAGED_CTX)
def test_paged_families_equal_fp64_causal_attention(ctx, dh):
    for T in U.PAGED_T:
        for family in U.FAMILIES:
            c = U.paged_case(family, ctx, T, dh)
            assert (c.rows.sum(1) == np.asarray(U.paged_lens(T))).all()


def test_families_tell_a_future_key_and_a_lost_diagonal():
    """what the closed forms are for: one key too many or the diagonal key lost moves `latest` to another V row"""
    c = U.dense_case("latest", "none", 65, 64)
    for shift in (1, -1):        # query i answering as query i + 1 (a future key counted) / i - 1 (the diagonal lost)
        other = np.roll(c.exp, -shift, axis=1)
        assert float(np.abs(other - c.exp)[:, 1:-1].max()) >= 0.125


@pytest.fixture(scope="module")
def tiny():
    sd = synth.decoder_state_dict(5, 97, 48, 64, 2)
    return sd, DecoderRef(sd, n_head=2)


def test_causal_ref_with_every_switch_off_is_the_oracle(tiny):
    sd, ref = tiny
    off = U.CausalRef(sd, n_head=2, true_pos=False, causal_mask=False, feed_once=False)
    idx = torch.from_numpy(synth.integers(6, "causal_host", (3, 20), 0, 97)).long()
    valid = torch.arange(20)[None, :] < torch.tensor([20, 7, 1])[:, None]
    for nv in (None, valid):
        a, ca, va = ref.forward(idx, None, None, nv)
        b, cb, vb = off.forward(idx, None, None, nv)
        assert torch.equal(a, b) and torch.equal(va, vb)
        a2, _, _ = ref.forward(idx[:, :1], ca, va)
        b2, _, _ = off.forward(idx[:, :1], cb, vb)
        assert torch.equal(a2, b2)
    prompts = [[1, 5, 14], [2], [1, 7, 20, 33, 34]]
    w, wl = ref.generate_greedy(prompts, 6, return_logits=True)
    g, gl = off.generate_greedy(prompts, 6, return_logits=True)
    assert w == g and torch.equal(wl, gl)


def test_causal_ref_ignores_the_future(tiny):
    sd, _ = tiny
    ref = U.CausalRef(sd, n_head=2)
    idx = torch.from_numpy(synth.integers(7, "causal_host", (2, 24), 0, 97)).long()
    base, _, _ = ref.forward(idx)
    for t in (0, 11, 22):
        other = idx.clone()
        other[:, t + 1:] = (other[:, t + 1:] + 13) % 97
        lg, _, _ = ref.forward(other)
        assert torch.equal(lg[:, :t + 1], base[:, :t + 1])
        assert not torch.equal(lg[:, t + 1:], base[:, t + 1:])
    # and the unmasked reference does not: the control
    un = U.CausalRef(sd, n_head=2, causal_mask=False)
    other = idx.clone()
    other[:, 12:] = (other[:, 12:] + 13) % 97
    assert not torch.equal(un.forward(other)[0][:, :12], un.forward(idx)[0][:, :12])


def test_causal_ref_cached_and_uncached_agree(tiny):
    sd, _ = tiny
    ref = U.CausalRef(sd, n_head=2)
    idx = torch.from_numpy(synth.integers(8, "causal_host", (2, 30), 0, 97)).long()
    whole, _, _ = ref.forward(idx)
    for a in (1, 13):
        l0, cache, cv = ref.forward(idx[:, :a])
        l1, _, _ = ref.forward(idx[:, a:], cache, cv)
        assert float((torch.cat([l0, l1], 1) - whole).abs().max()) < 1e-5
    # token by token, ragged: each row equals its solo prefill
    lens = [30, 9]
    valid = torch.arange(30)[None, :] < torch.tensor(lens)[:, None]
    rag, _, _ = ref.forward(idx, None, None, valid)
    for b, n in enumerate(lens):
        solo, _, _ = ref.forward(idx[b:b + 1, :n])
        assert float((rag[b, :n] - solo[0]).abs().max()) < 1e-5


def test_greedy_feeds_every_token_once(tiny):
    """generate_greedy of the causal reference = argmax of the one-shot causal forward over prompt + what it generated"""
    sd, _ = tiny
    ref = U.CausalRef(sd, n_head=2)
    prompts = [[3], [1, 5], [1, 7, 20, 33, 34]]
    outs, sl = ref.generate_greedy(prompts, 8, return_logits=True)
    for b, p in enumerate(prompts):
        full = torch.tensor(outs[b][:-1]).view(1, -1)
        lg, _, _ = ref.forward(full)
        assert float((lg[0, len(p) - 1:] - sl[b]).abs().max()) < 1e-5


def test_step_logits_are_the_rows_of_one_masked_forward(tiny):
    """causal_step_logits (prefill without the last token, feed it, feed the ids) = ONE masked forward over prompt + fed at positions
    len - 1 + s, to the 1e-5 the cached and the uncached CausalRef are held to; a one-token prompt prefills nothing"""
    sd, _ = tiny
    ref = U.CausalRef(sd, n_head=2)
    prompts = [[3], [1, 5], [1, 7, 20, 33, 34], [int(v) for v in synth.integers(9, "causal_host", (30,), 0, 97)]]
    fed = [[int(v) for v in row] for row in synth.integers(10, "causal_host", (4, 8), 0, 97)]
    got = U.causal_step_logits(ref, prompts, fed)
    assert got.shape == (4, 8, 97) and got.dtype == torch.float32
    assert U.CausalSteps(ref, prompts).rows[0] == [None, None]
    for b, p in enumerate(prompts):
        whole, _, _ = ref.forward(torch.tensor([p + fed[b][:-1]]))
        assert float((whole[0, len(p) - 1:] - got[b]).abs().max()) < 1e-5


def test_step_logits_with_every_switch_off_are_oracle_logps(tiny):
    """the reference-mode loop the other generation tests hard-code (prefill the whole prompt, re-feed its last token): bit for bit"""
    from test_gpu_guidance import oracle_logps
    sd, ref = tiny
    off = U.CausalRef(sd, n_head=2, true_pos=False, causal_mask=False, feed_once=False)
    prompts = [[3], [1, 5], [1, 7, 20, 33, 34]]
    fed = [[int(v) for v in row] for row in synth.integers(11, "causal_host", (3, 6), 0, 97)]
    got = U.causal_step_logits(off, prompts, fed)
    for b, p in enumerate(prompts):
        assert torch.equal(torch.log_softmax(got[b].double(), dim=1), oracle_logps(ref, p, fed[b]))


def test_walk_without_a_form_is_generate_greedy(tiny):
    sd, _ = tiny
    ref = U.CausalRef(sd, n_head=2)
    prompts = [[3], [1, 5], [1, 7, 20, 33, 34]]
    want, sl = ref.generate_greedy(prompts, 8, return_logits=True)
    res = U.walk(ref, [[p] for p in prompts], [(1.0,)] * 3, 8)
    assert [p + ids for p, ids in zip(prompts, res["ids"])] == want
    lp = torch.log_softmax(sl.double(), -1).gather(2, torch.tensor(res["ids"])[..., None])[..., 0]
    assert float((lp - torch.from_numpy(res["logprobs"])).abs().max()) < 1e-5


@pytest.mark.parametrize("name", U.FORMS)
@pytest.mark.parametrize("kind", ["tiny", "fused"])
def test_form_cases_meet_their_input_conditions(kind, name):
    """what test_gpu_causal_forms.py assumes of its inputs (causal_util.input_conditions): greedy top-2 gaps of at least
    5 x W x F32_TOL at every (row, step), so the GPU tests demand exact ids; the placed forced ids and the mixes move the checked values
    by ten bounds.  The 5-token prompt's last id occurs nowhere else in it."""
    groups, weights, _ = U.form_case(kind, name)
    prompts = U.form_prompts(kind, U.FORM_SEEDS[kind, name])
    assert [len(p) for p in prompts] == list(U.FORM_LENS) and prompts[2][-1] not in prompts[2][:-1]
    assert [g[0] for g in groups] == (prompts[1:] if name == "composed" else prompts)
    assert U.F32_TOL == 2e-4 and list(U.gap_floor(weights)) == [5 * U.mix_weight(w) * 2e-4 for w in weights]
    assert U.input_conditions(kind, name) == []
    if name in ("penalty", "bias", "grammar", "guided", "blended", "cpen"):
        forced, res = U.draw_forced(kind, name)
        _, _, form = U.form_case(kind, name)
        assert all(len(f) == U.FORM_STEPS and min(f) >= 0 for f in forced) and np.isfinite(res["choice"]).all()
        assert form.eos is None or all(e not in f for e, f in zip(form.eos, forced))


def test_forced_ids_place_the_last_prompt_id_and_its_class():
    from test_gpu_class_penalty import map12
    for kind in ("tiny", "fused"):
        forced, _ = U.draw_forced(kind, "penalty")
        groups, _, _ = U.form_case(kind, "penalty")
        assert forced[2][0] == groups[2][0][-1]
        forced, _ = U.draw_forced(kind, "cpen")
        groups, _, form = U.form_case(kind, "cpen")
        placed = 0
        for b, g in enumerate(groups):
            c = form.class_of[g[0][-1]]
            if c >= 0:
                assert form.class_of[forced[b][0]] == c and forced[b][0] != g[0][-1]
                placed += 1
        assert placed >= 2 and np.array_equal(form.class_of, map12(len(form.class_of)))


def test_prefill_lens_rule():
    """lens_m1: every prompt without its last token; a prompt of one token prefills nothing; off: the lengths themselves"""
    assert U.CausalRef.prefill_lens([1, 2, 5, 65]) == [0, 1, 4, 64]
    assert U.CausalRef.prefill_lens([1, 2, 5, 65], feed_once=False) == [1, 2, 5, 65]
    assert max(U.CausalRef.prefill_lens([1, 1])) == 0
