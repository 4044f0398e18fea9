// plan_generation (csrc/gen_plan.h) on the CPU: for the limits of a tiny engine, the StepKind and the flags every kind of request
// plans to, the KV reservation, and every refusal with its status and the row its message names.  set_error is this file's own: it
// keeps the last message.  Built with -fsanitize=address,undefined and run by tests/test_devmem_host.py; exit status 0 = every check held.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../music-generation-emotion-adaptive_amd/csrc/gen_plan.h"

namespace {
int g_failures = 0;
char g_msg[512] = "";
}  // namespace

namespace mgea {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}
}  // namespace mgea

using namespace mgea;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_msg); \
            ++g_failures;                                                        \
        }                                                                        \
    } while (0)

// a tiny engine: 100 ids, 8 rows, 128 tokens = 2 pages of context, no window, no grammar
const GenLimits kTiny{100, 8, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0};
GenLimits windowed(GenLimits c) { c.win_S = 1; c.win_R = 2; c.win_max_steps = 1000; return c; }   // 3 pages = 192 tokens
GenLimits with_grammar(GenLimits c, int n_state) { c.gram_n_state = n_state; return c; }

mgea_row_sampler greedy_row() { return mgea_row_sampler{1.0f, 1, 0.f, 1.0f, -1, 0, 7u, 0u, 0u}; }
float g_lp[1];   // never dereferenced: a scored request is one with a logprobs_out

// B rows of greedy records over prompts of 5 tokens and 12 steps; the cases change what they are about
struct Req {
    std::vector<mgea_row_sampler> rows;
    std::vector<mgea_row_logits> lrows;
    std::vector<int32_t> starts;
    std::vector<mgea_row_guidance> guide;
    std::vector<mgea_row_schedule> sched;
    GenRequest q;
    explicit Req(int B) : rows((size_t)B, greedy_row()) {
        q.B = B; q.Tp = 5; q.n_steps = 12;
    }
    Req& with_lrows() { lrows.assign(rows.size(), mgea_row_logits{nullptr, 0, 0}); return *this; }
    Req& with_starts() { starts.assign(rows.size(), -1); return *this; }
    Req& with_guide() { guide.assign(rows.size(), mgea_row_guidance{-1, 0.f}); return *this; }
    Req& with_sched(int n_seg_max) {
        mgea_row_schedule one{};
        one.n_segments = 1;
        sched.assign(rows.size(), one);
        q.n_seg_max = n_seg_max;
        return *this;
    }
    const GenRequest& get() {
        q.rows = rows.empty() ? nullptr : rows.data();   // no records: the uniform form
        q.lrows = lrows.empty() ? nullptr : lrows.data();
        q.start_states = starts.empty() ? nullptr : starts.data();
        q.guide = guide.empty() ? nullptr : guide.data();
        q.sched = sched.empty() ? nullptr : sched.data();
        return q;
    }
};

GenPlan planned(Req& r, const GenLimits& c = kTiny) {
    GenPlan p{};
    g_msg[0] = 0;
    const int rc = plan_generation(r.get(), c, &p);
    CHECK(rc == MGEA_OK);
    return p;
}
// the call is refused with `code`, and its message holds `what` (the row it names, or the rule)
bool refused(Req& r, int code, const char* what, const GenLimits& c = kTiny) {
    GenPlan p{};
    g_msg[0] = 0;
    const int rc = plan_generation(r.get(), c, &p);
    return rc == code && strstr(g_msg, what) != nullptr;
}
bool is_kind(const GenPlan& p, StepForm form, bool scored = false, bool windowed = false, bool guided = false, bool scheduled = false) {
    return p.kind == StepKind{form, scored, windowed, guided, scheduled};
}
// two pairs in a batch of four: rows 0 and 1 with the shadow rows 2 and 3
Req guided_pairs() {
    Req r(4);
    r.with_guide();
    r.guide[0] = {2, 1.5f};
    r.guide[1] = {3, 0.f};
    return r;
}

int main() {
    // ---- the kind and the flags
    {   // all-greedy rows
        Req r(2);
        const GenPlan p = planned(r);
        CHECK(is_kind(p, StepForm::GREEDY) && !p.grammar && !p.biased && !p.any_penalty && !p.may_stop_early && !p.capped);
        CHECK(p.n_pairs == 0 && p.n_sched == 0 && p.reserve == 17);
    }
    {   // one sampled row; an EOS id or a budget below n_steps makes the loop poll
        Req r(2);
        r.rows[1].top_k = 50;
        CHECK(is_kind(planned(r), StepForm::SAMPLED) && !planned(r).may_stop_early);
        r.rows[0].eos_id = 3;
        CHECK(planned(r).may_stop_early);
        r.rows[0].eos_id = -1;
        r.rows[1].max_new_tokens = 12;
        CHECK(!planned(r).may_stop_early);
        r.rows[1].max_new_tokens = 11;
        CHECK(planned(r).may_stop_early && !planned(r).capped);
    }
    {   // one penalized row
        Req r(2);
        r.rows[0].repetition_penalty = 1.2f;
        const GenPlan p = planned(r);
        CHECK(is_kind(p, StepForm::PENALIZED) && p.any_penalty && !p.biased);
    }
    {   // one biased row: a min_new_tokens or a bias vector; records that set neither change nothing
        Req r(2);
        r.with_lrows();
        CHECK(is_kind(planned(r), StepForm::GREEDY) && !planned(r).biased);
        r.lrows[1].min_new_tokens = 2;
        CHECK(is_kind(planned(r), StepForm::BIASED) && planned(r).biased && !planned(r).any_penalty);
        r.lrows[1].min_new_tokens = 0;
        r.lrows[0].bias_dev = g_lp;
        r.rows[0].repetition_penalty = 0.9f;
        CHECK(is_kind(planned(r), StepForm::BIASED) && planned(r).biased && planned(r).any_penalty);
    }
    {   // grammar start states: any >= 0; all -1 is no grammar
        Req r(2);
        r.with_starts();
        CHECK(is_kind(planned(r, with_grammar(kTiny, 3)), StepForm::GREEDY) && !planned(r, with_grammar(kTiny, 3)).grammar);
        r.starts[1] = 2;
        const GenPlan p = planned(r, with_grammar(kTiny, 3));
        CHECK(is_kind(p, StepForm::GRAMMAR) && p.grammar && !p.biased);
    }
    {   // scored all-greedy takes SAMPLED; a scored sampled or penalized batch keeps its form
        Req r(2);
        r.q.logprobs_out = g_lp;
        CHECK(is_kind(planned(r), StepForm::SAMPLED, true));
        r.rows[0].repetition_penalty = 1.2f;
        CHECK(is_kind(planned(r), StepForm::PENALIZED, true));
    }
    {   // guided all-greedy takes SAMPLED
        Req r = guided_pairs();
        const GenPlan p = planned(r);
        CHECK(is_kind(p, StepForm::SAMPLED, false, false, true) && p.n_pairs == 2 && !p.capped && p.reserve == 17);
        r.guide[0].shadow_row = r.guide[1].shadow_row = -1;   // records without a pair: not guided
        CHECK(is_kind(planned(r), StepForm::GREEDY) && planned(r).n_pairs == 0);
    }
    {   // scheduled rows: more than one segment
        Req r(3);
        r.with_sched(3);
        CHECK(is_kind(planned(r), StepForm::GREEDY) && planned(r).n_sched == 0);
        r.sched[1].n_segments = 3;
        r.sched[1].threshold[0] = 4;
        r.sched[1].threshold[1] = 4;   // equal thresholds are ascending
        r.sched[2].n_segments = 2;
        const GenPlan p = planned(r);
        CHECK(is_kind(p, StepForm::GREEDY, false, false, false, true) && p.n_sched == 2);
    }
    {   // the windowed variants: every kind, with the window's token count reserved and nothing capped however long the call
        const GenLimits w = windowed(kTiny);
        Req r(2);
        r.q.n_steps = 500;
        GenPlan p = planned(r, w);
        CHECK(is_kind(p, StepForm::GREEDY, false, true) && p.reserve == 192 && !p.capped && !p.may_stop_early);
        r.q.logprobs_out = g_lp;
        r.rows[0].top_k = 0;
        CHECK(is_kind(planned(r, w), StepForm::SAMPLED, true, true));
        Req g = guided_pairs();
        g.q.n_steps = 500;
        p = planned(g, w);
        CHECK(is_kind(p, StepForm::SAMPLED, false, true, true) && p.reserve == 192 && !p.capped);
        Req s(2);
        s.with_sched(2);
        s.sched[0].n_segments = 2;
        CHECK(is_kind(planned(s, w), StepForm::GREEDY, false, true, false, true) && planned(s, w).reserve == 192);
        Req u(2);   // the uniform form under a window
        const mgea_sampler_config sc{1.0f, 1, 0.f, -1, 0u};
        u.rows.clear();
        u.q.sampler = &sc;
        u.q.n_steps = 500;
        CHECK(is_kind(planned(u, w), StepForm::GREEDY, false, true) && planned(u, w).reserve == 192);
        // the window's own refusals: a prompt that does not fit the sink with one token to spare, more steps than max_steps
        r.q.Tp = 64;
        CHECK(refused(r, MGEA_ECAPACITY, "sink", w));
        r.q.Tp = 5;
        r.q.n_steps = 1001;
        CHECK(refused(r, MGEA_ECAPACITY, "max_steps", w));
    }
    {   // the uniform form
        Req u(2);
        u.rows.clear();
        mgea_sampler_config sc{1.0f, 1, 0.f, -1, 0u};
        u.q.sampler = &sc;
        GenPlan p = planned(u);
        CHECK(is_kind(p, StepForm::GREEDY) && !p.may_stop_early && !p.capped && p.reserve == 17);
        sc.top_k = 50;
        sc.eos_id = 2;
        u.q.penalty = 1.3f;
        p = planned(u);
        CHECK(is_kind(p, StepForm::PENALIZED) && p.any_penalty && p.may_stop_early);
        u.q.n_steps = 124;   // 5 + 124 > 128: the uniform form is never capped
        CHECK(refused(u, MGEA_ECAPACITY, "exceeds max_ctx"));
        sc.temperature = 0.f;
        u.q.n_steps = 12;
        CHECK(refused(u, MGEA_EINVAL, "temperature"));
    }

    // ---- reserve
    {   // clamped to max_ctx: the rows are capped there, and the loop polls for the rows that stop
        Req r(2);
        r.q.n_steps = 128;
        const GenPlan p = planned(r);
        CHECK(p.reserve == 128 && p.capped && p.may_stop_early);
        r.q.n_steps = 123;   // 5 + 123 = max_ctx: the last size that is not
        CHECK(planned(r).reserve == 128 && !planned(r).capped && !planned(r).may_stop_early);
        r.q.n_steps = 129;
        CHECK(refused(r, MGEA_ECAPACITY, "exceed max_ctx"));
    }
    {   // equal to the window's token count, whatever the call's size
        Req r(2);
        r.q.n_steps = 0;
        CHECK(planned(r, windowed(kTiny)).reserve == 192);
        r.q.n_steps = 1000;
        CHECK(planned(r, windowed(kTiny)).reserve == 192);
    }

    // ---- refusals: status, and the row the message names
    {   // a shadow of a shadow
        Req r = guided_pairs();
        r.guide[2] = {3, 1.f};
        r.guide[1] = {-1, 0.f};
        CHECK(refused(r, MGEA_EINVAL, "row 0: its shadow row 2 is conditional itself"));
    }
    {   // a row that is shadow to two rows
        Req r = guided_pairs();
        r.guide[1].shadow_row = 2;
        CHECK(refused(r, MGEA_EINVAL, "row 1: row 2 is already the shadow of row 0"));
    }
    {   // a self-shadow
        Req r = guided_pairs();
        r.guide[1].shadow_row = 1;
        CHECK(refused(r, MGEA_EINVAL, "row 1: a row cannot be its own shadow"));
    }
    {   // a negative scale
        Req r = guided_pairs();
        r.guide[1].scale = -0.5f;
        CHECK(refused(r, MGEA_EINVAL, "row 1: scale"));
    }
    {   // a capped guided call without a window; with one it is planned
        Req r = guided_pairs();
        r.q.n_steps = 124;
        CHECK(refused(r, MGEA_ECAPACITY, "a guided generation is never capped"));
        CHECK(planned(r, windowed(kTiny)).n_pairs == 2);
    }
    {   // descending thresholds
        Req r(2);
        r.with_sched(3);
        r.sched[1].n_segments = 3;
        r.sched[1].threshold[0] = 5;
        r.sched[1].threshold[1] = 3;
        CHECK(refused(r, MGEA_EINVAL, "row 1: thresholds not ascending"));
    }
    {   // a scheduled shadow row
        Req r = guided_pairs();
        r.with_sched(2);
        r.sched[3].n_segments = 2;
        CHECK(refused(r, MGEA_EINVAL, "row 3 is a guidance shadow row"));
    }
    {   // key 1 without a grammar; with one, on a row without a start state
        Req r(2);
        r.with_sched(2);
        r.sched[0].n_segments = 2;
        r.sched[0].key = 1;
        CHECK(refused(r, MGEA_EINVAL, "row 0: key 1 (grammar state) but no grammar is set"));
        CHECK(refused(r, MGEA_EINVAL, "row 0: key 1 (grammar state) on a row without a start state", with_grammar(kTiny, 3)));
        r.with_starts();
        r.starts[0] = 1;
        CHECK(is_kind(planned(r, with_grammar(kTiny, 3)), StepForm::GRAMMAR, false, false, false, true));
    }
    {   // Tp beyond a page when scheduled; unscheduled records leave the width alone
        Req r(2);
        r.with_sched(2);
        r.q.Tp = 65;
        CHECK(planned(r).n_sched == 0);
        r.sched[1].n_segments = 2;
        CHECK(refused(r, MGEA_ECAPACITY, "exceeds one page"));
        r.q.Tp = 64;
        CHECK(planned(r).n_sched == 1);
    }
    {   // a start state out of range
        Req r(2);
        r.with_starts();
        r.starts[1] = 3;
        CHECK(refused(r, MGEA_EINVAL, "row 1: start state 3 outside [0, 3)", with_grammar(kTiny, 3)));
        CHECK(refused(r, MGEA_EINVAL, "row 1 has start state 3 but no grammar is set"));
        r.starts[1] = -2;
        CHECK(refused(r, MGEA_EINVAL, "row 1: start state -2", with_grammar(kTiny, 3)));
    }
    {   // max_new_tokens greater than n_steps
        Req r(2);
        r.rows[1].max_new_tokens = 13;
        CHECK(refused(r, MGEA_EINVAL, "row 1: max_new_tokens 13 outside [0, 12]"));
    }
    {   // a bad logits record, a batch beyond max_batch, the other block mode
        Req r(2);
        r.with_lrows();
        r.lrows[1].min_new_tokens = 13;
        CHECK(refused(r, MGEA_EINVAL, "row 1: min_new_tokens 13"));
        Req big(9);
        CHECK(refused(big, MGEA_ECAPACITY, "batch 9 exceeds max_batch 8"));
        Req post(2);
        GenLimits c = kTiny;
        c.block_mode = MGEA_BLOCK_POSTLN_RELU;
        CHECK(refused(post, MGEA_EINVAL, "KV-cache block mode", c));
    }

    if (g_failures) return 1;
    puts("gen_plan ok");
    return 0;
}
