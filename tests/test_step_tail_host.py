"""The premises of tests/test_gpu_step_tail.py, proved on the CPU (tests/step_tail_util.py): the written rule reproduces the
reference's sampler loop and the oracle's id layout, the scenario table reaches every branch of the rule, the 'exact' inputs are exact
in fp32, and every partial-argmax row has exactly one acceptable answer."""
import numpy as np
import torch

import step_tail_util as U


def drive(tokens, eos, max_new=None, cap=None, prompt_len=3, n_steps=None):
    """the rule over a whole generation of one row that is offered tokens[t] at step t -> (ids_out, final state, n_done)"""
    n_steps = len(tokens) if n_steps is None else n_steps
    fed, length, done, step, n_done = 99, prompt_len, 0, 0, 0
    ids_out = [None] * n_steps
    for tok in tokens:
        r = U.end_of_step(tok, step, fed, length, done, eos, max_new, cap, n_steps)
        if r.entry is not None:
            ids_out[step] = r.entry
        fed, length, done, step, n_done = r.cur_id, r.ctx_len, r.done, r.row_step, n_done + r.n_done
        assert (r.fed, r.next_len) == (fed, length)
    return ids_out, (fed, length, done, step), n_done


def reference_loop(tokens, end_id):
    """api_cache.py:179-182 of the reference: append the drawn id, stop at [END_SEQUENCE]"""
    generated = []
    for next_id in tokens:
        generated.append(next_id)
        if next_id == end_id:
            break
    return generated


def test_rule_reproduces_the_reference_loop():
    rs = np.random.RandomState(5)
    for trial in range(200):
        tokens = rs.randint(0, 12, size=rs.randint(1, 20)).tolist()
        end_id = int(rs.randint(-1, 12))
        want = reference_loop(tokens, end_id)
        ids, (fed, length, done, step), n_done = drive(tokens, end_id)
        assert ids == want + [-1] * (len(tokens) - len(want))
        stopped = want[-1] == end_id
        assert (done, n_done) == ((1, 1) if stopped else (0, 0))
        assert fed == want[-1] and length == 3 + len(want) and step == len(tokens)


def test_rule_reproduces_the_oracle_id_layout():
    """oracle/decoder_ref.py generate_greedy appends one id per step and never stops: the rule without EOS gives the same ids, and
    with an EOS id the same ids up to the stop and -1 after it."""
    from mgea import synth
    from oracle.decoder_ref import DecoderRef
    sd = synth.decoder_state_dict(7, 48, 32, 64, 1)
    prompts = [[1, 5, 14], [2, 9]]
    n = 10
    outs = DecoderRef(sd, n_head=2).generate_greedy(prompts, n)
    for p, o in zip(prompts, outs):
        new = o[len(p):]
        assert len(new) == n
        ids, (_, length, done, _), _ = drive(new, -1, prompt_len=len(p))
        assert ids == new and done == 0 and length == len(p) + n
        eos = new[n // 2]
        stop = new.index(eos)
        ids, (_, length, done, _), n_done = drive(new, eos, prompt_len=len(p))
        assert ids == new[:stop + 1] + [-1] * (n - stop - 1) and (done, n_done) == (1, 1) and length == len(p) + stop + 1


def test_budget_cap_and_parking_over_a_generation():
    toks = list(range(10, 22))
    ids, (fed, length, done, step), n_done = drive(toks, -1, max_new=4, prompt_len=3)
    assert ids == toks[:4] + [-1] * 8 and (fed, length, done, step, n_done) == (13, 7, 1, 12, 1)
    # pages full when the budget ends: parked one position short, its later steps move nothing but row_step
    ids, (fed, length, done, step), n_done = drive(toks, -1, max_new=4, cap=7, prompt_len=3)
    assert ids == toks[:4] + [-1] * 8 and (fed, length, done, step, n_done) == (13, 6, 2, 12, 1)
    # a cap alone stops nothing, and a budget already behind the row never fires
    assert drive(toks, -1, cap=5)[1][2] == 0
    r = U.end_of_step(5, 7, 1, 4, 0, -1, 3, None, 20)
    assert (r.done, r.n_done) == (0, 0)


def test_scenario_table_reaches_every_branch():
    for records in (True, False):
        table = U.scenario_table(records)
        assert len(table) == (3 * 3 * 4 * 4 * 3 if records else 3 * 2 * 3) and len(table) <= 512
        sc = U.scenarios(len(table), records)
        assert sorted(map(str, sc["entries"])) == sorted(map(str, table)), "B = len(table) must see every combination once"
        for eos in ((U.EOS, -1) if not records else (None,)):
            ex = U.expected_state(sc, records, eos_by_value=eos)
            core = [t - set(U.COLUMN_TAGS) - {"records", "by_value"} for t in ex["tags"]]
            need = U.REQUIRED_TAG_SETS if records else [s for s in U.REQUIRED_TAG_SETS if not s & {"budget", "park", "past_budget", "full_but_running"}]
            if not records and eos == -1:
                need = [s for s in need if "eos" not in s]
            for req in need:
                for col in U.COLUMN_TAGS:
                    n = sum(1 for c, t in zip(core, ex["tags"]) if c == frozenset(req) and col in t)
                    assert n >= 1, f"records={records} eos={eos}: no scenario takes {sorted(req)} at {col}"
            # finishing rows of every kind, parked rows among them, and rows that were parked before
            assert ex["n_done"] == sum(1 for t in ex["tags"] if t & {"finish", "park"})
            assert (ex["n_done"] > 0) == (records or eos == U.EOS)   # (without records and without an EOS id nothing can finish)
            if records:
                combos = {(e["done"], e["tok"], e["budget"], e["cap"], e["step"]) for e in sc["entries"]}
                assert len(combos) == len(table)
    # the batch sizes of the GPU test: every axis value appears by B = 64, every combination by B = 512
    sc = U.scenarios(512, True)
    assert len({str(e) for e in sc["entries"]}) == 432
    sc = U.scenarios(64, True)
    for axis, values in (("done", U.DONES), ("tok", U.TOKS), ("budget", U.BUDGETS), ("cap", U.CAPS), ("step", U.STEPS)):
        assert {e[axis] for e in sc["entries"]} == set(values)


def test_scenario_numbers_mean_what_their_names_say():
    sc = U.scenarios(432, True)
    for j, e in enumerate(sc["entries"]):
        step, length, mx, cap = (int(sc[k][j]) for k in ("step", "len", "max_new", "cap"))
        assert {"lt": step + 1 < mx, "eq": step + 1 == mx, "gt": step + 1 > mx >= 1, "none": mx == 0}[e["budget"]]
        assert {"lt": length + 1 < cap < U.NONE, "eq": length + 1 == cap, "gt": length + 1 > cap >= 1, "none": cap == U.NONE}[e["cap"]]
        assert {"inner": step < U.N_STEPS - 1, "last": step == U.N_STEPS - 1, "beyond": step >= U.N_STEPS}[e["step"]]
        assert (sc["tok"][j] == sc["eos"][j]) == (e["tok"] == "eos") and (sc["eos"][j] == -1) == (e["tok"] == "no_eos")
        assert length >= 1 and sc["tok"][j] != sc["fed"][j]


def test_exact_inputs_are_exact_in_fp32():
    for nt in U.TILE_COUNTS:
        pval, pidx, _ = U.argmax_inputs(nt)
        finite = pval[np.isfinite(pval)]
        assert pval.dtype == np.float32 and (finite == np.round(finite)).all() and np.abs(finite).max() < 2 ** 24
        assert (finite.astype(np.float64).astype(np.float32) == finite).all()
    # the planted logits of the sampler rows and the score values: small integers and dyadic fractions
    for v in (U.WIN, 0.0, -8.0, 0.25, -3.5):
        assert float(np.float32(v)) == v
    assert torch.tensor([U.POISON], dtype=torch.int32).view(torch.float32).isnan().all()


def test_argmax_rows_have_exactly_one_answer():
    for nt in U.TILE_COUNTS:
        pval, pidx, names = U.argmax_inputs(nt)
        want, ok = U.argmax_rule(pval, pidx)
        assert ok, "two maximal tiles with one id"
        assert len(names) == len(want) >= len(U.winner_tiles(nt)) + 2
        for r, name in enumerate(names):
            assert len(set(pidx[r].tolist())) == nt, "pidx is a permutation of distinct ids"
            v = pval[r]
            if name.startswith("winner@"):
                w = int(name.split("@")[1])
                assert want[r] == pidx[r, w] and (np.delete(v, w) < U.WIN).all()
            elif name.startswith("tie:"):
                at = np.flatnonzero(v == U.WIN)
                assert len(at) == 2 and want[r] == pidx[r, at[1]] < pidx[r, at[0]], "the lower id sits in the later tile"
            elif name == "all-inf":
                assert want[r] == pidx[r].min()
            elif name == "all-nan":
                assert want[r] == 0
            elif name == "nan-ignored":
                assert np.isnan(v).any() and np.isnan(v[int(np.argmin(pidx[r]))]) and want[r] == pidx[r, nt // 2]
        # the rows tell tile order from id order: the first and the last maximal tile, and the lowest id overall, are other answers somewhere
        first = np.asarray([pidx[r, int(np.nanargmax(np.where(np.isnan(pval[r]), -np.inf, pval[r])))] for r in range(len(want)) if names[r] != "all-nan"])
        w2 = np.asarray([want[r] for r in range(len(want)) if names[r] != "all-nan"])
        if nt >= 3:
            assert (first != w2).any()
        assert U.winner_tiles(257) == [0, 63, 64, 127, 128, 191, 192, 255, 256]


def test_tiled_offsets_are_a_bijection_and_match_the_layout_comment():
    for M, N in ((64, 32), (130, 128), (5, 1024)):
        off = U.tiled_offsets(M, N)
        assert len(np.unique(off)) == M * N and off.max() < U.tiled_floats(M, N)
    off = U.tiled_offsets(64, 1028)
    assert len(np.unique(off)) == 64 * 1028 and 64 * 1028 <= off.max() < U.tiled_floats(64, 1028)   # past 64 * N: one row group only
    off = U.tiled_offsets(33, 4)
    assert len(np.unique(off)) == 33 * 4 and off.max() < U.tiled_floats(33, 4) == 2048
    # (row 17, k 44): group 0, chunk 1, [17 / 16 = 1][(44 / 4) % 2 = 1][(44 / 8) % 4 * 16 + 17 % 16 = 17], element 0
    assert U.tiled_offsets(64, 64)[17, 44] == 2048 + ((1 * 2 + 1) * 64 + 17) * 4


def test_side_rules():
    assert U.presence_bit_set(31, 0, 32) and not U.presence_bit_set(32, 0, 32) and not U.presence_bit_set(5, 1, 32) and not U.presence_bit_set(-1, 0, 32)
    assert U.score_entry(3, 0, 0.25, 4) == (3, 0.25) and U.score_entry(3, 2, 0.25, 4) == (3, 0.0) and U.score_entry(4, 0, 0.25, 4) is None
    assert U.embed_position(70, 1, 64) == 63 and U.embed_position(70, 0, 64) == 0 and U.embed_id(-3, 50) == 0 and U.embed_id(50, 50) == 49
