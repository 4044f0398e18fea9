// What a generation is asked for (GenRequest), which launch sequence its steps take (StepKind) and everything the host decides before
// the first launch (GenPlan): plan_generation holds every refusal of mgea_decoder_generate* that needs no device, in one order, and
// derives the plan from the host records alone; do_generate (decoder_generate.hip) runs exactly that plan.  Plain C++17, no HIP include and no
// handle: tests/native/gen_plan_test.cpp compiles it for the host alone.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/mgea.h"

namespace mgea {

void set_error(const char* fmt, ...);   // the thread-local message behind mgea_last_error (capi.hip)

#define MGEA_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            ::mgea::set_error(__VA_ARGS__);      \
            return (code);                       \
        }                                        \
    } while (0)

#define MGEA_TRY(expr)               \
    do {                             \
        int _rc = (expr);            \
        if (_rc != MGEA_OK) return _rc; \
    } while (0)

// The tail of a decode step -- everything after the LM head -- has five launch sequences, and a generation runs one of them on every step:
//   GREEDY (every row has top_k == 1)  the head leaves per-tile (max, argmax) partials and no logits row; an argmax tail merges them
//   SAMPLED                            the head writes the logits row; the plain sampler draws from it
//   PENALIZED (a row's penalty != 1)   as SAMPLED with the PENALTY sampler over the rows' presence bitmaps, which the tail keeps up to
//                                      date; a greedy row is top_k = 1 of its penalized row (the head's partials know no penalty)
//   BIASED (a row's bias or min_new)   as PENALIZED with the BIAS sampler and the rows' bias buffer (a penalty of 1 changes nothing)
//   GRAMMAR (a row's start state >= 0) as BIASED with the GRAMMAR sampler: the row's automaton state masks the classes its table bans
//                                      and the sampler's bookkeeping thread moves the state on (GrammarArgs, common.h)
enum class StepForm { GREEDY = 0, SAMPLED, PENALIZED, BIASED, GRAMMAR };
inline StepForm step_form(bool all_greedy, bool any_penalized, bool any_biased) {
    return any_biased ? StepForm::BIASED : any_penalized ? StepForm::PENALIZED : all_greedy ? StepForm::GREEDY : StepForm::SAMPLED;
}
inline bool form_has_presence(StepForm f) { return f == StepForm::PENALIZED || f == StepForm::BIASED || f == StepForm::GRAMMAR; }
inline bool form_has_bias(StepForm f) { return f == StepForm::BIASED || f == StepForm::GRAMMAR; }

// One launch sequence of a decode step, and so the key of the captured step graphs next to the batch and the step count: every other
// setting of a request lives in the rows' device records.
//   scored     the scored sampler (never with the GREEDY form: scoring needs the logits row)
//   windowed   the step opens with the KV window's evict launch and files into the windowed histories (kv_window.hip)
//   guided     the guidance-mix launch over the logits, between the head and the sampler (guidance.hip; never GREEDY)
//   scheduled  behind the evict launch, the launch that applies the rows' prompt schedules (recondition.hip)
//   truncated  the truncating sampler over the rows' mgea_row_truncation records (BIASED or GRAMMAR form only)
//   blended    the blend-mix launch over the logits, next to the guidance mix (blend.hip; never GREEDY)
//   class_penalized  the class-penalty launch over the logits, behind the two mixes (class_penalty.hip; never GREEDY)
struct StepKind {
    StepForm form;
    bool scored = false, windowed = false, guided = false, scheduled = false, truncated = false, blended = false;
    bool class_penalized = false;   // trailing and defaulted: StepKind is aggregate-initialised
    bool operator==(const StepKind& o) const {
        return form == o.form && scored == o.scored && windowed == o.windowed && guided == o.guided && scheduled == o.scheduled &&
               truncated == o.truncated && blended == o.blended && class_penalized == o.class_penalized;
    }
};

// host check of rows[0, B) (mgea_decoder_generate_rows, mgea_op_sample_rows): MGEA_EINVAL naming the first bad row; n_steps < 0 skips the
// budget check
inline int check_row_samplers(const mgea_row_sampler* rows, int B, int V, int n_steps, const char* who) {
    MGEA_REQUIRE(rows, MGEA_EINVAL, "%s: rows is NULL", who);
    for (int b = 0; b < B; ++b) {
        const mgea_row_sampler& r = rows[b];
        MGEA_REQUIRE(std::isfinite(r.temperature) && r.temperature > 0.f, MGEA_EINVAL, "%s: row %d: temperature must be finite and > 0 (got %g)",
                     who, b, (double)r.temperature);
        MGEA_REQUIRE(r.top_k >= 0 && r.top_k <= V, MGEA_EINVAL, "%s: row %d: top_k %d outside [0, %d]", who, b, r.top_k, V);
        MGEA_REQUIRE(std::isfinite(r.repetition_penalty) && r.repetition_penalty > 0.f, MGEA_EINVAL,
                     "%s: row %d: repetition_penalty must be finite and > 0 (got %g)", who, b, (double)r.repetition_penalty);
        MGEA_REQUIRE(n_steps < 0 || (r.max_new_tokens >= 0 && r.max_new_tokens <= n_steps), MGEA_EINVAL,
                     "%s: row %d: max_new_tokens %d outside [0, %d]", who, b, r.max_new_tokens, n_steps);
    }
    return MGEA_OK;
}
// host check of the rows' mgea_row_logits records: reserved == 0, 0 <= min_new_tokens <= n_steps (n_steps < 0: no upper bound)
inline int check_row_logits(const mgea_row_logits* lrows, int B, int n_steps, const char* who) {
    for (int b = 0; b < B; ++b) {
        const mgea_row_logits& l = lrows[b];
        MGEA_REQUIRE(l.reserved == 0, MGEA_EINVAL, "%s: row %d: mgea_row_logits.reserved must be 0", who, b);
        MGEA_REQUIRE(l.min_new_tokens >= 0 && (n_steps < 0 || l.min_new_tokens <= n_steps), MGEA_EINVAL,
                     "%s: row %d: min_new_tokens %d outside [0, %d]", who, b, l.min_new_tokens, n_steps < 0 ? 0x7fffffff : n_steps);
    }
    return MGEA_OK;
}
// What checked rows [B] (+ lrows [B] or NULL) say about the batch.  The form: greedy only if every row is, penalized if any row is (p = 1
// rows are unchanged by it: x * 1, x / 1 exact), biased if any row has a bias or a min_new_tokens.  may_stop_early: some row has an EOS
// id or a budget below n_steps.
struct RowRecords { StepForm form; bool any_penalty; bool may_stop_early; };
inline RowRecords row_records(const mgea_row_sampler* rows, const mgea_row_logits* lrows, int B, int n_steps) {
    bool all_greedy = true, pen = false, biased = false, stop = false;
    for (int b = 0; b < B; ++b) {
        all_greedy = all_greedy && rows[b].top_k == 1;
        pen = pen || rows[b].repetition_penalty != 1.0f;
        stop = stop || rows[b].eos_id >= 0 || (rows[b].max_new_tokens > 0 && rows[b].max_new_tokens < n_steps);
        if (lrows) biased = biased || lrows[b].bias_dev || lrows[b].min_new_tokens > 0;
    }
    return RowRecords{step_form(all_greedy, pen, biased), pen, stop};
}

// host check of guide[0, B) (mgea_decoder_generate_rows_guided): MGEA_EINVAL naming the first bad row; *n_pairs = the conditional rows
inline int check_row_guidance(const mgea_row_guidance* guide, int B, int* n_pairs) {
    const char* who = "decoder_generate_rows_guided";
    *n_pairs = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t u = guide[b].shadow_row;
        MGEA_REQUIRE(u >= -1 && u < B, MGEA_EINVAL, "%s: row %d: shadow_row %d outside [-1, %d)", who, b, u, B);
        MGEA_REQUIRE(u != b, MGEA_EINVAL, "%s: row %d: a row cannot be its own shadow", who, b);
        if (u < 0) continue;
        MGEA_REQUIRE(std::isfinite(guide[b].scale) && guide[b].scale >= 0.f, MGEA_EINVAL, "%s: row %d: scale %g must be finite and >= 0", who, b,
                     (double)guide[b].scale);
    }
    std::vector<int> owner((size_t)B, -1);   // the conditional row of every shadow
    for (int b = 0; b < B; ++b) {
        const int32_t u = guide[b].shadow_row;
        if (u < 0) continue;
        MGEA_REQUIRE(guide[u].shadow_row < 0, MGEA_EINVAL, "%s: row %d: its shadow row %d is conditional itself (shadow_row %d)", who, b, u,
                     guide[u].shadow_row);
        MGEA_REQUIRE(owner[(size_t)u] < 0, MGEA_EINVAL, "%s: row %d: row %d is already the shadow of row %d", who, b, u, owner[(size_t)u]);
        owner[(size_t)u] = b;
        *n_pairs += 1;
    }
    return MGEA_OK;
}

// host check of sched[0, B) (mgea_decoder_generate_rows_scheduled): MGEA_EINVAL naming the first bad row; *n_sched = the rows with
// more than one segment
inline int check_row_schedules(const mgea_row_schedule* sched, int B, int n_seg_max, const int32_t* start_states, int gram_n_state,
                               const mgea_row_guidance* guide, int* n_sched) {
    const char* who = "decoder_generate_rows_scheduled";
    *n_sched = 0;
    std::vector<char> shadow((size_t)B, 0);
    for (int b = 0; guide && b < B; ++b)
        if (guide[b].shadow_row >= 0 && guide[b].shadow_row < B) shadow[(size_t)guide[b].shadow_row] = 1;
    for (int b = 0; b < B; ++b) {
        const mgea_row_schedule& r = sched[b];
        MGEA_REQUIRE(r.n_segments >= 1 && r.n_segments <= MGEA_SCHEDULE_MAX_SEGMENTS, MGEA_EINVAL, "%s: row %d: n_segments %d outside [1, %d]", who, b,
                     r.n_segments, MGEA_SCHEDULE_MAX_SEGMENTS);
        MGEA_REQUIRE(r.n_segments <= n_seg_max, MGEA_EINVAL, "%s: row %d: n_segments %d exceeds n_seg_max %d", who, b, r.n_segments, n_seg_max);
        MGEA_REQUIRE(r.key == 0 || r.key == 1, MGEA_EINVAL, "%s: row %d: key %d (0 = step index, 1 = grammar state)", who, b, r.key);
        MGEA_REQUIRE(r.reserved == 0, MGEA_EINVAL, "%s: row %d: reserved must be 0", who, b);
        for (int s = 0; s + 1 < r.n_segments; ++s) {
            MGEA_REQUIRE(r.threshold[s] >= 0, MGEA_EINVAL, "%s: row %d: threshold[%d] = %d is negative", who, b, s, r.threshold[s]);
            MGEA_REQUIRE(s == 0 || r.threshold[s] >= r.threshold[s - 1], MGEA_EINVAL, "%s: row %d: thresholds not ascending (%d after %d)", who, b,
                         r.threshold[s], r.threshold[s - 1]);
        }
        if (r.n_segments == 1) continue;
        MGEA_REQUIRE(!shadow[(size_t)b], MGEA_EINVAL, "%s: row %d is a guidance shadow row: it has one segment (its prompt has no emotion tokens)", who, b);
        if (r.key == 1) {
            MGEA_REQUIRE(gram_n_state > 0, MGEA_EINVAL, "%s: row %d: key 1 (grammar state) but no grammar is set", who, b);
            MGEA_REQUIRE(start_states && start_states[b] >= 0, MGEA_EINVAL, "%s: row %d: key 1 (grammar state) on a row without a start state", who, b);
        }
        *n_sched += 1;
    }
    return MGEA_OK;
}

// Does the record switch a stage on?  (0 = off; typical_p == 1 is off too: everything weighs 1)
inline bool truncation_on(const mgea_row_truncation& t) {
    return t.min_p > 0.f || (t.typical_p > 0.f && t.typical_p < 1.f) || t.epsilon_cutoff > 0.f || t.eta_cutoff > 0.f;
}
// host check of trunc[0, B) (mgea_decoder_generate_rows_truncated, mgea_op_sample_rows_truncated): MGEA_EINVAL naming the first bad row;
// *n_rows = the non-greedy rows (rows NULL: all rows) with a stage switched on
inline int check_row_truncation(const mgea_row_truncation* trunc, const mgea_row_sampler* rows, int B, const char* who, int* n_rows) {
    *n_rows = 0;
    for (int b = 0; b < B; ++b) {
        const mgea_row_truncation& t = trunc[b];
        MGEA_REQUIRE(std::isfinite(t.min_p) && t.min_p >= 0.f && t.min_p <= 1.f, MGEA_EINVAL, "%s: row %d: min_p %g outside [0, 1]", who, b,
                     (double)t.min_p);
        MGEA_REQUIRE(std::isfinite(t.typical_p) && t.typical_p >= 0.f && t.typical_p <= 1.f, MGEA_EINVAL, "%s: row %d: typical_p %g outside [0, 1]",
                     who, b, (double)t.typical_p);
        MGEA_REQUIRE(std::isfinite(t.epsilon_cutoff) && t.epsilon_cutoff >= 0.f && t.epsilon_cutoff < 1.f, MGEA_EINVAL,
                     "%s: row %d: epsilon_cutoff %g outside [0, 1)", who, b, (double)t.epsilon_cutoff);
        MGEA_REQUIRE(std::isfinite(t.eta_cutoff) && t.eta_cutoff >= 0.f && t.eta_cutoff < 1.f, MGEA_EINVAL,
                     "%s: row %d: eta_cutoff %g outside [0, 1)", who, b, (double)t.eta_cutoff);
        if (truncation_on(t) && !(rows && rows[b].top_k == 1)) *n_rows += 1;
    }
    return MGEA_OK;
}

// host check of blend[0, B) (mgea_decoder_generate_rows_blended): MGEA_EINVAL naming the first bad row; *n_groups = the groups, *n_rows
// = the grouped rows.  guide and sched (each NULL = absent) have passed their own checks.
inline int check_row_blend(const mgea_row_blend* blend, int B, const mgea_row_guidance* guide, const mgea_row_schedule* sched, int* n_groups,
                           int* n_rows) {
    const char* who = "decoder_generate_rows_blended";
    *n_groups = *n_rows = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t l = blend[b].leader;
        MGEA_REQUIRE(l >= -1 && l < B, MGEA_EINVAL, "%s: row %d: leader %d outside [-1, %d)", who, b, l, B);
        if (l < 0) continue;
        MGEA_REQUIRE(blend[l].leader == l, MGEA_EINVAL, "%s: row %d: its leader row %d does not name itself (leader %d)", who, b, l,
                     blend[l].leader);
        MGEA_REQUIRE(std::isfinite(blend[b].weight), MGEA_EINVAL, "%s: row %d: weight %g must be finite", who, b, (double)blend[b].weight);
    }
    std::vector<char> paired((size_t)B, 0);   // conditional and shadow rows of the guidance pairs
    for (int b = 0; guide && b < B; ++b)
        if (guide[b].shadow_row >= 0 && guide[b].shadow_row < B) paired[(size_t)b] = paired[(size_t)guide[b].shadow_row] = 1;
    std::vector<int> size((size_t)B, 0);
    std::vector<double> sum((size_t)B, 0.0);
    for (int b = 0; b < B; ++b) {
        const int32_t l = blend[b].leader;
        if (l < 0) continue;
        MGEA_REQUIRE(!paired[(size_t)b], MGEA_EINVAL, "%s: row %d is in a blend group and in a guidance pair", who, b);
        MGEA_REQUIRE(!sched || sched[b].n_segments == 1, MGEA_EINVAL, "%s: row %d is in a blend group and has %d segments (a grouped row has one)",
                     who, b, sched ? sched[b].n_segments : 1);
        size[(size_t)l] += 1;
        MGEA_REQUIRE(size[(size_t)l] <= MGEA_BLEND_MAX_ROWS, MGEA_EINVAL, "%s: row %d: the group of leader row %d has more than %d rows", who, b,
                     l, MGEA_BLEND_MAX_ROWS);
        sum[(size_t)l] += (double)blend[b].weight;
        *n_rows += 1;
    }
    for (int b = 0; b < B; ++b) {
        if (blend[b].leader != b) continue;
        MGEA_REQUIRE(size[(size_t)b] >= 2, MGEA_EINVAL, "%s: row %d: a group of %d row (a group has 2 to %d)", who, b, size[(size_t)b],
                     MGEA_BLEND_MAX_ROWS);
        MGEA_REQUIRE(std::fabs(sum[(size_t)b] - 1.0) <= 1e-3, MGEA_EINVAL,
                     "%s: row %d: the weights of its group sum to %g, not 1 (a blend is an affine combination)", who, b, sum[(size_t)b]);
        *n_groups += 1;
    }
    return MGEA_OK;
}

// Is the record on?  (a row that is off is never written: class_penalty.hip)
inline bool class_penalty_on(const mgea_row_class_penalty& r) { return r.frequency != 0.f || r.presence != 0.f; }
// host check of cpen[0, B) (mgea_decoder_generate_rows_class_penalized, mgea_op_class_penalty): MGEA_EINVAL naming the first bad row;
// *n_rows = the rows that are on.  n_steps < 0 skips the check of window == 0 against the steps; n_class = the engine's map (0 = none).
inline int check_row_class_penalty(const mgea_row_class_penalty* cpen, int B, int n_steps, int n_class, const char* who, int* n_rows) {
    *n_rows = 0;
    for (int b = 0; b < B; ++b) {
        const mgea_row_class_penalty& r = cpen[b];
        MGEA_REQUIRE(std::isfinite(r.frequency) && std::fabs(r.frequency) <= 1e4f, MGEA_EINVAL,
                     "%s: row %d: frequency %g must be finite and within +-1e4", who, b, (double)r.frequency);
        MGEA_REQUIRE(std::isfinite(r.presence) && std::fabs(r.presence) <= 1e4f, MGEA_EINVAL,
                     "%s: row %d: presence %g must be finite and within +-1e4", who, b, (double)r.presence);
        MGEA_REQUIRE(r.window >= 0 && r.window <= MGEA_CLASS_PENALTY_MAX_WINDOW, MGEA_EINVAL, "%s: row %d: window %d outside [0, %d]", who, b,
                     r.window, MGEA_CLASS_PENALTY_MAX_WINDOW);
        MGEA_REQUIRE(r.reserved == 0, MGEA_EINVAL, "%s: row %d: mgea_row_class_penalty.reserved must be 0", who, b);
        if (!class_penalty_on(r)) continue;
        MGEA_REQUIRE(r.window > 0 || n_steps <= MGEA_CLASS_PENALTY_MAX_WINDOW, MGEA_EINVAL,
                     "%s: row %d: window 0 (the whole history) with %d steps: above %d steps a row that is on needs a window", who, b, n_steps,
                     MGEA_CLASS_PENALTY_MAX_WINDOW);
        MGEA_REQUIRE(n_class > 0, MGEA_EINVAL, "%s: row %d has a class penalty but no class map is set (set_penalty_classes)", who, b);
        *n_rows += 1;
    }
    return MGEA_OK;
}

// Everything a generation is asked for.  prompt_ids, lens, forced and the three outputs are DEVICE memory, as in the C ABI; the records
// are host memory.
struct GenRequest {
    const char* who = "decoder_generate";   // the entry point's name, in front of its own messages
    const int32_t* prompt_ids = nullptr;    // [B][Tp]; scheduled: [n_seg_max][B][Tp]
    const int32_t* lens = nullptr;          // [B] or NULL: every prompt has Tp tokens
    int B = 0, Tp = 0, n_steps = 0;
    // the uniform form (rows == NULL): `sampler` and `penalty` on every row; penalty == 1: none, exactly the unpenalized launch sequence
    const mgea_sampler_config* sampler = nullptr;
    float penalty = 1.0f;
    // the per-row form: rows [B], and with it only, each NULL = absent and then every launch is what it is without it --
    // lrows [B] the rows' logit bias and min_new_tokens; start_states [B] their grammar start states (-1 = none; any >= 0 makes it the
    // GRAMMAR form); guide [B] their guidance pairs (any shadow_row >= 0 makes it guided); sched [B] their prompt schedules over
    // n_seg_max prompt variants (any n_segments > 1 makes it scheduled; variant 0 is the prompt)
    const mgea_row_sampler* rows = nullptr;
    const mgea_row_logits* lrows = nullptr;
    const int32_t* start_states = nullptr;
    const mgea_row_guidance* guide = nullptr;
    const mgea_row_schedule* sched = nullptr;
    int n_seg_max = 1;
    const mgea_row_truncation* trunc = nullptr;   // [B] the rows' truncation records (any non-greedy row with a stage on makes it truncated)
    const mgea_row_blend* blend = nullptr;        // [B] the rows' blend groups (any leader >= 0 makes it blended)
    const mgea_row_class_penalty* cpen = nullptr; // [B] the rows' class penalties (any record that is on makes it class-penalised)
    const int32_t* forced = nullptr;        // [B][n_steps] ids the rows must take, -1 = free (scored only)
    int32_t* ids_out = nullptr;             // [B][n_steps]
    float* logprobs_out = nullptr;          // [B][n_steps]; not NULL makes the generation scored
    float* choice_out = nullptr;            // [B][n_steps] or NULL (scored only)
    bool scored() const { return logprobs_out != nullptr; }
};

// What the checks need to know about the handle.  win_S == 0: no KV window is set.
struct GenLimits {
    int vocab, max_batch, max_ctx, block_mode;
    int win_S, win_R, win_max_steps;
    int gram_n_state;
    int cpen_n_class = 0;   // the n_class of the penalty class map (mgea_decoder_set_penalty_classes); 0: none is set
};

// What the host decides about a generation before its first launch.
struct GenPlan {
    StepKind kind;
    bool grammar;          // some row has a start state
    bool biased;           // the rows' own form is BIASED (a bias vector or a min_new_tokens)
    bool any_penalty;      // some row's penalty != 1
    bool may_stop_early;   // some row can finish before n_steps: the launch loop polls for it
    bool capped;           // rows stop where their KV pages end (launch_clamp_budgets, parking)
    int n_pairs;           // guidance pairs: conditional rows with a shadow row
    int n_sched;           // scheduled rows: more than one prompt variant
    int n_trunc;           // truncated rows: non-greedy rows with a truncation stage switched on
    bool truncated;        // n_trunc > 0: the steps run the truncating sampler
    int reserve;           // tokens of KV pages every row gets
    int n_groups;          // blend groups: leaders
    int n_blend_rows;      // rows in a blend group, leaders included
    int n_cpen;            // rows whose class-penalty record is on
};

// Every host check of a generation, then its plan.  Calls no HIP function and touches no handle.
inline int plan_generation(const GenRequest& q, const GenLimits& c, GenPlan* out) {
    const int B = q.B, Tp = q.Tp, n_steps = q.n_steps;
    MGEA_REQUIRE(c.block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "decoder_generate needs the KV-cache block mode");
    MGEA_REQUIRE(n_steps >= 0 && Tp > 0, MGEA_EINVAL, "decoder_generate: bad n_steps / Tp");
    RowRecords rr;
    GenPlan p{};
    p.reserve = Tp + n_steps;
    // With a window set every generation is windowed: P pages per row, no budget clamp, no parking, every page id through the table.
    const bool windowed = c.win_S > 0;
    if (windowed) {
        MGEA_REQUIRE(B > 0 && B <= c.max_batch, MGEA_ECAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
        MGEA_REQUIRE(Tp + 1 <= c.win_S * MGEA_KV_PAGE_TOKENS, MGEA_ECAPACITY,
                     "prompt width %d + 1 exceeds the window's sink of %d pages (%d tokens)", Tp, c.win_S, c.win_S * MGEA_KV_PAGE_TOKENS);
        MGEA_REQUIRE(n_steps <= c.win_max_steps, MGEA_ECAPACITY, "%d steps exceed the window's max_steps %d", n_steps, c.win_max_steps);
        p.reserve = (c.win_S + c.win_R) * MGEA_KV_PAGE_TOKENS;
    }
    if (q.rows) {
        MGEA_REQUIRE(B > 0 && B <= c.max_batch, MGEA_ECAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
        MGEA_TRY(check_row_samplers(q.rows, B, c.vocab, n_steps, "decoder_generate_rows"));
        if (q.lrows) MGEA_TRY(check_row_logits(q.lrows, B, n_steps, "decoder_generate_rows"));
        for (int b = 0; q.start_states && b < B; ++b) {
            const int32_t s0 = q.start_states[b];
            if (s0 == -1) continue;
            MGEA_REQUIRE(s0 >= 0, MGEA_EINVAL, "decoder_generate_rows_grammar: row %d: start state %d (-1 = none)", b, s0);
            MGEA_REQUIRE(c.gram_n_state > 0, MGEA_EINVAL, "decoder_generate_rows_grammar: row %d has start state %d but no grammar is set", b, s0);
            MGEA_REQUIRE(s0 < c.gram_n_state, MGEA_EINVAL, "decoder_generate_rows_grammar: row %d: start state %d outside [0, %d)", b, s0,
                         c.gram_n_state);
            p.grammar = true;
        }
        if (q.trunc) MGEA_TRY(check_row_truncation(q.trunc, q.rows, B, "decoder_generate_rows_truncated", &p.n_trunc));
        p.truncated = p.n_trunc > 0;
        if (q.guide) MGEA_TRY(check_row_guidance(q.guide, B, &p.n_pairs));
        if (q.sched) {   // (n_seg_max itself: checked by the entry point)
            MGEA_TRY(check_row_schedules(q.sched, B, q.n_seg_max, q.start_states, c.gram_n_state, q.guide, &p.n_sched));
            MGEA_REQUIRE(p.n_sched == 0 || Tp <= MGEA_KV_PAGE_TOKENS, MGEA_ECAPACITY,
                         "decoder_generate_rows_scheduled: prompt width %d exceeds one page of %d tokens", Tp, MGEA_KV_PAGE_TOKENS);
        }
        if (q.blend) MGEA_TRY(check_row_blend(q.blend, B, q.guide, q.sched, &p.n_groups, &p.n_blend_rows));
        if (q.cpen)
            MGEA_TRY(check_row_class_penalty(q.cpen, B, n_steps, c.cpen_n_class, "decoder_generate_rows_class_penalized", &p.n_cpen));
        // A guided pair must run the same steps: rows stopped where their pages end (launch_clamp_budgets) would get budgets of their own
        // prompt lengths.  Under a window nothing is clamped, and each row of a pair evicts on its own schedule.
        MGEA_REQUIRE(p.n_pairs == 0 || windowed || Tp + n_steps <= c.max_ctx, MGEA_ECAPACITY,
                     "decoder_generate_rows_guided: prompt width %d + %d steps exceed max_ctx %d (a guided generation is never capped; set a window)",
                     Tp, n_steps, c.max_ctx);
        // (and so must the rows of a blend group)
        MGEA_REQUIRE(p.n_groups == 0 || windowed || Tp + n_steps <= c.max_ctx, MGEA_ECAPACITY,
                     "decoder_generate_rows_blended: prompt width %d + %d steps exceed max_ctx %d (a blended generation is never capped; set a window)",
                     Tp, n_steps, c.max_ctx);
        // every row needs lens[b] + its budget; rows past the reservation are stopped there on the device (launch_clamp_budgets)
        // (a window holds every row for as long as it runs: nothing to stop)
        MGEA_REQUIRE(windowed || (Tp < c.max_ctx && n_steps <= c.max_ctx), MGEA_ECAPACITY, "prompt width %d / %d steps exceed max_ctx %d", Tp,
                     n_steps, c.max_ctx);
        if (!windowed) p.reserve = p.reserve < c.max_ctx ? p.reserve : c.max_ctx;
        rr = row_records(q.rows, q.lrows, B, n_steps);
    } else {
        MGEA_REQUIRE(windowed || Tp + n_steps <= c.max_ctx, MGEA_ECAPACITY, "prompt %d + %d steps exceeds max_ctx %d", Tp, n_steps, c.max_ctx);
        MGEA_REQUIRE(q.sampler->temperature > 0.f, MGEA_EINVAL, "temperature must be > 0");
        rr = RowRecords{step_form(q.sampler->top_k == 1, q.penalty != 1.0f, false), q.penalty != 1.0f, q.sampler->eos_id >= 0};
    }
    p.capped = !windowed && p.reserve < Tp + n_steps;
    p.may_stop_early = rr.may_stop_early || p.capped;
    p.any_penalty = rr.any_penalty;
    p.biased = rr.form == StepForm::BIASED;
    const bool scored = q.scored(), guided = p.n_pairs > 0, blended = p.n_groups > 0, cpen = p.n_cpen > 0;
    // scoring, guidance, blends and class penalties need the logits row: all-greedy rows run as top_k == 1 records of the SAMPLED form (the exact argmax, ties to
    // the lowest id)
    // truncation lives in the <PENALTY, BIAS> sampler family, as the grammar does: the BIASED form at least (bitmaps over every row, a
    // penalty of 1 and a record without bias_on change nothing)
    const StepForm form = p.grammar           ? StepForm::GRAMMAR
                          : p.truncated     ? StepForm::BIASED
                          : (scored || guided || blended || cpen) && rr.form == StepForm::GREEDY ? StepForm::SAMPLED
                                              : rr.form;
    p.kind = StepKind{form, scored, windowed, guided, p.n_sched > 0, p.truncated, blended, cpen};
    *out = p;
    return MGEA_OK;
}

// Which row's inputs each row of a planned generation runs on, -1 = its own.  A non-leader member of a blend group takes its leader's,
// otherwise a guidance shadow row its conditional row's (a row is never both: check_row_blend).  Same inputs -- records, bias vector,
// forced ids, presence bitmap --, same id.  guide / blend: the request's records, NULL = absent.
inline std::vector<int> mirror_sources(const mgea_row_guidance* guide, const mgea_row_blend* blend, int B) {
    std::vector<int> src((size_t)B, -1);
    for (int b = B - 1; guide && b >= 0; --b)   // (descending: of two rows naming one shadow, which the plan refuses, the lower would win)
        if (guide[b].shadow_row >= 0 && guide[b].shadow_row < B) src[(size_t)guide[b].shadow_row] = b;
    for (int u = 0; blend && u < B; ++u)
        if (blend[u].leader >= 0 && blend[u].leader != u) src[(size_t)u] = blend[u].leader;
    return src;
}

}  // namespace mgea
