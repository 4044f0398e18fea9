"""Host side of the end-of-step tests (tests/test_gpu_step_tail.py, checked by tests/test_step_tail_host.py): the WRITTEN RULE of one
row's step end, the rules that hang on it (presence bit, score filing, embedding position), the scenario table that
reaches every branch of the rule, and the partial-argmax inputs.  numpy / CPU torch only, no device code.

THE RULE (restated from the contract above end_row_step in csrc/common.h, not from its body).  A row enters the end of a step with
    tok   the id the step produced          step  the index of the step it is producing (row_step)
    fed   the id it was fed (cur_ids)       len   its ctx_len          done  0 running, 1 finished, 2 finished and parked
    eos, max_new, cap   its EOS id (-1 none), its step budget and the tokens its pages hold (NONE = no limit); without records the
                        launch's one eos holds and there is neither budget nor cap
  * a running row APPENDS tok: ids_out[step] = tok, cur_ids = tok, ctx_len = len + 1;
  * it FINISHES if tok is its EOS id or this was its last budgeted step (step + 1 == max_new): done = 1 and the launch's n_done + 1;
  * a row that finishes with its pages full (the new ctx_len >= cap) is PARKED instead: done = 2, ctx_len stays len, n_done + 1 too;
  * a finished or parked row appends nothing: ids_out[step] = -1, cur_ids, ctx_len and done stay;
  * row_step = step + 1 either way; ids_out is written only while step < n_steps;
  * the next step feeds the row's cur_ids at position ctx_len (both as left above)."""
import math
from collections import namedtuple

import numpy as np

NONE = 0x7FFFFFFF          # no budget / no cap (the records' INT32_MAX)
POISON = 0x7FC5A5A5        # mgea.ops.POISON_BITS
N_STEPS = 6                # ids_out columns of the scenario launches
EOS = 2
TOL = 2e-5                 # the project's fp32 row-operation bound

StepEnd = namedtuple("StepEnd", "cur_id ctx_len done row_step entry n_done fed next_len tags")


def end_of_step(tok, step, fed, length, done, eos, max_new, cap, n_steps):
    """One row's step end by THE RULE.  entry: what ids_out[step] receives, None = not written.  tags: the branches taken."""
    tags = {"records" if (max_new, cap) != (None, None) else "by_value"}
    max_new = NONE if max_new is None else max_new
    cap = NONE if cap is None else cap
    if done:
        tags.add("was_finished" if done == 1 else "was_parked")
        cur, new_len, new_done, entry, inc = fed, length, done, -1, 0
    else:
        tags.add("append")
        cur, new_len, new_done, entry, inc = tok, length + 1, 0, tok, 0
        by_eos, by_budget = tok == eos, step + 1 == max_new
        if by_eos:
            tags.add("eos")
        if by_budget:
            tags.add("budget")
        if by_eos or by_budget:
            inc = 1
            if new_len >= cap:
                tags.add("park")
                new_done, new_len = 2, length
            else:
                tags.add("finish")
                new_done = 1
        else:
            tags.add("runs_on")
            if step + 1 > max_new:
                tags.add("past_budget")       # a budget already behind the row never fires
            if new_len >= cap:
                tags.add("full_but_running")  # the cap alone finishes nothing
    if step < n_steps:
        tags.add("last_column" if step == n_steps - 1 else "inner_column")
    else:
        tags.add("beyond_ids_out")
        entry = None
    return StepEnd(cur, new_len, new_done, step + 1, entry, inc, cur, new_len, frozenset(tags))


def presence_bit_set(tok, done, V):
    """the row's bitmap gains bit tok & 31 of word tok >> 5 iff the row was running at step start and tok is an id of the vocabulary"""
    return (not done) and 0 <= tok < V


def score_entry(step, done, value, stride):
    """(index, value) the histories receive, None = nothing filed: at the row's step, 0 for a row that was already finished"""
    return None if step >= stride else (step, 0.0 if done else value)


def embed_position(next_len, absolute_pos, pos_rows):
    return min(next_len if absolute_pos else 0, pos_rows - 1)


def embed_id(fed, vocab):
    return min(max(fed, 0), vocab - 1)


# ---- the scenario table --------------------------------------------------------------------------------------------------------
DONES = (0, 1, 2)
TOKS = ("eos", "other", "no_eos")
BUDGETS = ("lt", "eq", "gt", "none")
CAPS = ("lt", "eq", "gt", "none")
STEPS = ("inner", "last", "beyond")


def scenario_table(records):
    """Every combination, as dicts of names.  Without records a launch has one eos and no budgets or caps: the token axis is then
    'is the launch's EOS value or not', and the launch is run with eos = EOS and with eos = -1."""
    if records:
        return [dict(done=d, tok=t, budget=bu, cap=c, step=s) for d in DONES for t in TOKS for bu in BUDGETS for c in CAPS for s in STEPS]
    return [dict(done=d, tok=t, budget="none", cap="none", step=s) for d in DONES for t in TOKS[:2] for s in STEPS]


def scenarios(B, records, n_steps=N_STEPS, max_len=120):
    """B rows of a launch: row j takes table entry (j * stride) mod len(table), stride coprime to the table's length, so that any B
    sees every axis value early and B >= len(table) sees every combination.  Returns a dict of int64 arrays [B]: tok, step, fed, len,
    done, eos, max_new (0 = none, as mgea_row_sampler.max_new_tokens), cap (NONE = none), plus the table entries."""
    table = scenario_table(records)
    stride = 175 if records else 7
    assert math.gcd(stride, len(table)) == 1
    out = {k: np.zeros(B, np.int64) for k in ("tok", "step", "fed", "len", "done", "eos", "max_new", "cap")}
    picked = []
    for j in range(B):
        e = table[(j * stride) % len(table)]
        picked.append(e)
        step = {"inner": 1 + j % 3, "last": n_steps - 1, "beyond": n_steps + j % 2}[e["step"]]
        length = 1 + (11 * j) % max_len
        tok = EOS if e["tok"] == "eos" else 3 + (5 * j) % 37
        out["tok"][j], out["step"][j], out["fed"][j], out["len"][j], out["done"][j] = tok, step, 40 + j % 9, length, e["done"]
        out["eos"][j] = -1 if e["tok"] == "no_eos" else EOS
        out["max_new"][j] = {"lt": step + 3, "eq": step + 1, "gt": step, "none": 0}[e["budget"]]
        out["cap"][j] = {"lt": length + 5, "eq": length + 1, "gt": length, "none": NONE}[e["cap"]]
    out["entries"] = picked
    return out


def expected_state(sc, records, eos_by_value=-1, n_steps=N_STEPS):
    """THE RULE on every row of scenarios(): dict of int64 arrays cur_ids, ctx_len, done, row_step, fed, next_len [B], ids_out
    [B, n_steps] (POISON where nothing is written), n_done (the launch's count), tags (list of frozensets), running (bool [B])."""
    B = len(sc["tok"])
    res = {k: np.zeros(B, np.int64) for k in ("cur_ids", "ctx_len", "done", "row_step", "fed", "next_len")}
    ids_out = np.full((B, n_steps), POISON, np.int64)
    n_done, tags = 0, []
    for j in range(B):
        eos = int(sc["eos"][j]) if records else eos_by_value
        max_new = (int(sc["max_new"][j]) or NONE) if records else None
        cap = int(sc["cap"][j]) if records else None
        r = end_of_step(int(sc["tok"][j]), int(sc["step"][j]), int(sc["fed"][j]), int(sc["len"][j]), int(sc["done"][j]), eos, max_new, cap, n_steps)
        res["cur_ids"][j], res["ctx_len"][j], res["done"][j], res["row_step"][j] = r.cur_id, r.ctx_len, r.done, r.row_step
        res["fed"][j], res["next_len"][j] = r.fed, r.next_len
        if r.entry is not None:
            ids_out[j, int(sc["step"][j])] = r.entry
        n_done += r.n_done
        tags.append(r.tags)
    res.update(ids_out=ids_out, n_done=n_done, tags=tags, running=np.asarray(sc["done"]) == 0)
    return res


# every tag combination of interest must be reached by the table (tests/test_step_tail_host.py counts them)
REQUIRED_TAG_SETS = [
    {"append", "eos", "finish"}, {"append", "budget", "finish"}, {"append", "eos", "budget", "finish"},
    {"append", "eos", "park"}, {"append", "budget", "park"}, {"append", "eos", "budget", "park"},
    {"append", "runs_on"}, {"append", "runs_on", "past_budget"}, {"append", "runs_on", "full_but_running"},
    {"was_finished"}, {"was_parked"},
]
COLUMN_TAGS = ("inner_column", "last_column", "beyond_ids_out")


# ---- the k-tiled activation layout (csrc/common.h, "k-tiled") --------------------------------------------------------------------
def tiled_offsets(M, N):
    """float offset of element (row, n) of a k-tiled [M, N] buffer -> int64 [M, N]: 64-row groups of 64 N floats, 32-wide k-chunks of
    2048 floats, inside a chunk the 16-byte group of (row, k..k+3) at [row / 16][(k / 4) % 2][(k / 8) % 4 * 16 + row % 16].
    (N % 32 != 0 leaves the last chunk partly used: such a buffer needs 64 * round_up(N, 32) floats and holds ONE row group.)"""
    row, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    r = row & 63
    return (row >> 6) * 64 * N + (n >> 5) * 2048 + (((((r >> 4) * 2 + ((n >> 2) & 1)) * 64 + ((n >> 3) & 3) * 16 + (r & 15)) << 2) + (n & 3))


from mgea.ops import tiled_floats  # noqa: E402  (one definition: the wrappers size their buffers by it)


# ---- partial argmax ----------------------------------------------------------------------------------------------------------
TILE_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 521, 1041)
WIN, BASE_MOD = 4096.0, 997


def winner_tiles(nt):
    """first and last tile, and the tiles either side of every multiple of 64 (every multiple of 256 is one)"""
    w = {0, nt - 1}
    for m in range(64, nt + 1, 64):
        w |= {m - 1} | ({m} if m < nt else set())
    return sorted(w)


def argmax_rule(pval, pidx):
    """The answer per row: the LOWEST id among the tiles that hold the row's maximum, NaN partials ignored; a row of only NaN gives 0.
    Returns (ids int64 [B], ok bool): ok is False if a row's answer is not unique (two maximal tiles with the same id)."""
    ids, ok = [], True
    for v, ix in zip(np.asarray(pval, np.float32), np.asarray(pidx, np.int64)):
        keep = ~np.isnan(v)
        if not keep.any():
            ids.append(0)
            continue
        best = v[keep].max()
        cand = ix[keep & (v == best)]
        ok = ok and len(set(cand.tolist())) == len(cand)
        ids.append(int(cand.min()))
    return np.asarray(ids, np.int64), ok


def argmax_inputs(nt, id_span=1200):
    """(pval fp32 [B, nt], pidx int32 [B, nt], names): one row per winner tile (the planted maximum WIN, everything else a distinct-ish
    integer below BASE_MOD), then the special rows.  pidx is a per-row permutation of nt distinct ids in [0, id_span): tile order
    says nothing about id order."""
    rows_v, rows_i, names = [], [], []
    rs = np.random.RandomState(1000 + nt)

    def fresh():
        v = ((np.arange(nt) * 7919 + len(rows_v)) % BASE_MOD).astype(np.float32)
        ix = rs.permutation(id_span)[:nt].astype(np.int32)
        return v, ix

    def tie(i1, i2, name):
        v, ix = fresh()
        v[i1] = v[i2] = WIN
        lo, hi = sorted((int(ix[i1]), int(ix[i2])))
        ix[i1], ix[i2] = hi, lo            # the lower id sits in the LATER tile
        rows_v.append(v), rows_i.append(ix), names.append(name)

    for w in winner_tiles(nt):
        v, ix = fresh()
        v[w] = WIN
        rows_v.append(v), rows_i.append(ix), names.append(f"winner@{w}")
    if nt >= 3:
        tie(1, 2, "tie:lanes")
    if nt >= 71:
        tie(3, 70, "tie:waves")            # lanes 3 and 6 of the 64-lane kernel; waves 0 and 1 of the 256-thread kernel
    if nt >= 200:
        tie(130, 199, "tie:waves23")       # waves 2 and 3
    if nt >= 5 + 256 + 1:
        tie(5, 5 + 256, "tie:same_thread")  # one thread of either kernel meets both
    v, ix = fresh()
    v[:] = -np.inf
    rows_v.append(v), rows_i.append(ix), names.append("all-inf")
    v, ix = fresh()
    v[:] = np.nan
    rows_v.append(v), rows_i.append(ix), names.append("all-nan")
    if nt >= 2:
        v, ix = fresh()
        v[nt // 2] = WIN
        if int(np.argmin(ix)) == nt // 2:          # the lowest id must sit under a NaN, not under the maximum
            ix[[nt // 2, (nt // 2 + 1) % nt]] = ix[[(nt // 2 + 1) % nt, nt // 2]]
        lowest = int(np.argmin(ix))
        nan_at = [t for t in {0, nt - 1, lowest} if t != nt // 2]
        v[nan_at] = np.nan
        rows_v.append(v), rows_i.append(ix), names.append("nan-ignored")
    return np.stack(rows_v), np.stack(rows_i), names


# ---- fp64 references of the row statistics -------------------------------------------------------------------------------------
def ln64(x, w=None, b=None, eps=1e-5):
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    y = (x - mean) / np.sqrt(var + eps)
    if w is not None:
        y = y * np.asarray(w, np.float64) + np.asarray(b, np.float64)
    return y


def ln_from_stats(x, mean, m2, eps=1e-5):
    """LayerNorm of x (no affine) in fp64 from a kernel's (mean, M2 = sum of squared deviations)"""
    x = np.asarray(x, np.float64)
    mean, m2 = np.asarray(mean, np.float64)[:, None], np.asarray(m2, np.float64)[:, None]
    return (x - mean) / np.sqrt(m2 / x.shape[-1] + eps)
