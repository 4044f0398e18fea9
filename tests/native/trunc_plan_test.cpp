// plan_generation (csrc/gen_plan.h) and the rows' truncation records (mgea_row_truncation) on the CPU: the refusals with the row
// their message names, truncated => the BIASED form at least, NULL or all-off records => the plan there was before, and the
// step-graph key.  set_error is this file's own: it keeps the last message.  Run by tests/test_truncation_host.py; exit status 0 and
// "trunc_plan ok" = every check held.
#include <math.h>
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

// a tiny engine: 100 ids, 8 rows, 128 tokens of context, no window; 3 grammar states where a case needs them
const GenLimits kTiny{100, 8, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0};
const GenLimits kGram{100, 8, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 3};

mgea_row_sampler row(int top_k, float penalty = 1.0f) { return mgea_row_sampler{1.0f, top_k, 0.f, penalty, -1, 0, 7u, 0u, 0u}; }
const mgea_row_truncation kOff{0.f, 0.f, 0.f, 0.f};
float g_lp[1];   // never dereferenced: a scored request is one with a logprobs_out

struct Req {
    std::vector<mgea_row_sampler> rows;
    std::vector<mgea_row_truncation> trunc;
    std::vector<mgea_row_logits> lrows;
    std::vector<int32_t> starts;
    std::vector<mgea_row_guidance> guide;
    GenRequest q;
    Req(int B, int top_k) : rows((size_t)B, row(top_k)) { q.B = B; q.Tp = 5; q.n_steps = 12; }
    Req& with_trunc(mgea_row_truncation t = kOff) { trunc.assign(rows.size(), t); return *this; }
    const GenRequest& get() {
        q.rows = rows.data();
        q.trunc = trunc.empty() ? nullptr : trunc.data();
        q.lrows = lrows.empty() ? nullptr : lrows.data();
        q.start_states = starts.empty() ? nullptr : starts.data();
        q.guide = guide.empty() ? nullptr : guide.data();
        return q;
    }
};

GenPlan planned(Req& r, const GenLimits& c = kTiny) {
    GenPlan p{};
    g_msg[0] = 0;
    CHECK(plan_generation(r.get(), c, &p) == MGEA_OK);
    return p;
}
bool refused(Req& r, const char* what) {
    GenPlan p{};
    g_msg[0] = 0;
    return plan_generation(r.get(), kTiny, &p) == MGEA_EINVAL && strstr(g_msg, what) != nullptr;
}
bool same_plan(const GenPlan& a, const GenPlan& b) {
    return a.kind == b.kind && a.grammar == b.grammar && a.biased == b.biased && a.any_penalty == b.any_penalty &&
           a.may_stop_early == b.may_stop_early && a.capped == b.capped && a.n_pairs == b.n_pairs && a.n_sched == b.n_sched &&
           a.reserve == b.reserve && a.truncated == b.truncated && a.n_trunc == b.n_trunc;
}

int main() {
    // ---- NULL or all-off records: the plan there was before, form by form
    for (int top_k : {1, 50}) {
        for (float pen : {1.0f, 1.3f}) {
            Req plain(3, top_k), off(3, top_k);
            plain.rows[1].repetition_penalty = off.rows[1].repetition_penalty = pen;
            off.with_trunc();
            off.trunc[2].typical_p = 1.0f;   // 1 is off too
            const GenPlan a = planned(plain), b = planned(off);
            CHECK(same_plan(a, b) && !b.truncated && !b.kind.truncated && b.n_trunc == 0);
        }
    }
    {   // a greedy row ignores its record: an all-greedy batch stays on the greedy head
        Req r(2, 1);
        r.with_trunc(mgea_row_truncation{0.1f, 0.5f, 1e-3f, 1e-3f});
        const GenPlan p = planned(r);
        CHECK(p.kind.form == StepForm::GREEDY && !p.truncated && !p.kind.truncated);
    }
    // ---- truncated => the BIASED form at least, whatever the rows' own form is; GRAMMAR with a start state
    const mgea_row_truncation one_stage[4] = {{0.05f, 0, 0, 0}, {0, 0.9f, 0, 0}, {0, 0, 3e-4f, 0}, {0, 0, 0, 2e-3f}};
    for (const mgea_row_truncation& t : one_stage) {
        Req r(3, 1);
        r.rows[1].top_k = 50;   // rows 0 and 2 greedy
        r.with_trunc();
        r.trunc[1] = t;
        r.trunc[0] = t;   // on a greedy row: not counted
        const GenPlan p = planned(r);
        CHECK(p.truncated && p.kind.truncated && p.n_trunc == 1 && p.kind.form == StepForm::BIASED);
        CHECK(form_has_presence(p.kind.form) && form_has_bias(p.kind.form) && !p.biased && !p.any_penalty && !p.grammar);
    }
    {
        Req r(2, 0);
        r.rows[0].repetition_penalty = 1.2f;
        r.with_trunc(mgea_row_truncation{0.02f, 0.8f, 0, 0});
        GenPlan p = planned(r);
        CHECK(p.kind.form == StepForm::BIASED && p.any_penalty && !p.biased && p.n_trunc == 2);
        r.lrows.assign(2, mgea_row_logits{nullptr, 3, 0});
        p = planned(r);
        CHECK(p.kind.form == StepForm::BIASED && p.biased && p.kind.truncated);
        r.starts.assign(2, -1);
        r.starts[1] = 2;
        p = planned(r, kGram);
        CHECK(p.kind.form == StepForm::GRAMMAR && p.grammar && p.kind.truncated);
        r.q.logprobs_out = g_lp;
        p = planned(r, kGram);
        CHECK(p.kind.form == StepForm::GRAMMAR && p.kind.scored && p.kind.truncated);
    }
    {   // scored or guided all-sampled rows: BIASED, not SAMPLED
        Req r(4, 50);
        r.with_trunc(mgea_row_truncation{0, 0, 1e-3f, 0});
        r.guide.assign(4, mgea_row_guidance{-1, 0.f});
        r.guide[0] = {2, 1.5f};
        const GenPlan p = planned(r);
        CHECK(p.kind.form == StepForm::BIASED && p.kind.guided && p.kind.truncated && p.n_pairs == 1);
    }
    // ---- the step-graph key
    {
        Req a(2, 50), b(2, 50);
        b.rows[0].repetition_penalty = 1.1f;
        b.lrows.assign(2, mgea_row_logits{nullptr, 1, 0});   // b's own form is BIASED
        a.with_trunc(mgea_row_truncation{0.05f, 0, 0, 0});
        const GenPlan pa = planned(a), pb = planned(b);
        CHECK(pa.kind.form == pb.kind.form && !(pa.kind == pb.kind));
        StepKind k = pb.kind;
        k.truncated = true;
        CHECK(k == pa.kind);
        Req c(2, 50);
        c.with_trunc(mgea_row_truncation{0, 0.3f, 1e-4f, 0});   // other values, the same key
        CHECK(planned(c).kind == pa.kind);
    }
    // ---- the refusals, naming the first bad row
    {
        const float nan = NAN, inf = INFINITY;
        struct Bad { mgea_row_truncation t; const char* what; };
        const Bad bad[] = {{{-0.1f, 0, 0, 0}, "min_p"},        {{1.5f, 0, 0, 0}, "min_p"},          {{nan, 0, 0, 0}, "min_p"},
                           {{0, -0.5f, 0, 0}, "typical_p"},    {{0, 1.01f, 0, 0}, "typical_p"},     {{0, inf, 0, 0}, "typical_p"},
                           {{0, 0, -1e-3f, 0}, "epsilon_cutoff"}, {{0, 0, 1.0f, 0}, "epsilon_cutoff"}, {{0, 0, nan, 0}, "epsilon_cutoff"},
                           {{0, 0, 0, -1e-3f}, "eta_cutoff"},  {{0, 0, 0, 1.0f}, "eta_cutoff"},     {{0, 0, 0, inf}, "eta_cutoff"}};
        for (const Bad& c : bad) {
            Req r(3, 50);
            r.with_trunc();
            r.trunc[2] = c.t;
            CHECK(refused(r, "row 2") && strstr(g_msg, c.what) != nullptr);
            r.trunc[1] = c.t;
            CHECK(refused(r, "row 1"));
            r.rows[1].top_k = 1;   // a greedy row's record is checked too
            CHECK(refused(r, "row 1"));
        }
        Req ok(1, 50);
        ok.with_trunc(mgea_row_truncation{1.0f, 1.0f, 0.999f, 0.999f});   // the closed and the open ends
        CHECK(planned(ok).truncated);
        int n = -1;
        CHECK(check_row_truncation(ok.trunc.data(), nullptr, 1, "t", &n) == MGEA_OK && n == 1);
        CHECK(!truncation_on(kOff) && !truncation_on(mgea_row_truncation{0, 1.0f, 0, 0}));
    }
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("trunc_plan ok\n");
    return 0;
}
