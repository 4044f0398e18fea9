// plan_generation (csrc/gen_plan.h) and the rows' class-penalty records (mgea_row_class_penalty) on the CPU: a row that is on =>
// kind.class_penalized and never the GREEDY form; the flag next to scored, windowed, guided, scheduled, truncated and blended; NULL or
// all-off records => the blended plan there was before, field for field; the step-graph key; the refusals with the row their message
// names.  set_error is this file's own: it keeps the last message.  Run by tests/test_class_penalty_host.py; exit status 0 and
// "class_penalty_plan ok" = every check held.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
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

// a tiny engine: 100 ids, 12 rows, 128 tokens of context, a map of 12 classes; the same without a map; the same with a window of
// 1 + 1 pages and 8192 steps
const GenLimits kTiny{100, 12, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0, 12};
const GenLimits kNoMap{100, 12, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0};
const GenLimits kWin{100, 12, 128, MGEA_BLOCK_PRELN_GELU, 1, 1, 8192, 0, 12};

mgea_row_sampler row(int top_k, float penalty = 1.0f) { return mgea_row_sampler{1.0f, top_k, 0.f, penalty, -1, 0, 7u, 0u, 0u}; }
const mgea_row_class_penalty kOff{0.f, 0.f, 0, 0};
float g_lp[1];   // never dereferenced: a scored request is one with a logprobs_out

struct Req {
    std::vector<mgea_row_sampler> rows;
    std::vector<mgea_row_truncation> trunc;
    std::vector<mgea_row_guidance> guide;
    std::vector<mgea_row_schedule> sched;
    std::vector<mgea_row_blend> blend;
    std::vector<mgea_row_class_penalty> cpen;
    GenRequest q;
    Req(int B, int top_k) : rows((size_t)B, row(top_k)) { q.B = B; q.Tp = 5; q.n_steps = 12; }
    Req& with_cpen() { cpen.assign(rows.size(), kOff); return *this; }
    Req& on(int b, float f, float p, int w) {
        if (cpen.empty()) with_cpen();
        cpen[(size_t)b] = mgea_row_class_penalty{f, p, w, 0};
        return *this;
    }
    const GenRequest& get() {
        q.rows = rows.data();
        q.trunc = trunc.empty() ? nullptr : trunc.data();
        q.guide = guide.empty() ? nullptr : guide.data();
        q.sched = sched.empty() ? nullptr : sched.data();
        q.blend = blend.empty() ? nullptr : blend.data();
        q.cpen = cpen.empty() ? nullptr : cpen.data();
        return q;
    }
};

GenPlan planned(Req& r, const GenLimits& c = kTiny) {
    GenPlan p{};
    g_msg[0] = 0;
    CHECK(plan_generation(r.get(), c, &p) == MGEA_OK);
    return p;
}
bool refused(Req& r, const char* row_name, const char* what, const GenLimits& c = kTiny, int code = MGEA_EINVAL) {
    GenPlan p{};
    g_msg[0] = 0;
    return plan_generation(r.get(), c, &p) == code && strstr(g_msg, row_name) != nullptr && strstr(g_msg, what) != nullptr &&
           strstr(g_msg, "decoder_generate_rows_class_penalized") != nullptr;
}
bool same_plan(const GenPlan& a, const GenPlan& b) {
    return a.kind == b.kind && a.grammar == b.grammar && a.biased == b.biased && a.any_penalty == b.any_penalty &&
           a.may_stop_early == b.may_stop_early && a.capped == b.capped && a.n_pairs == b.n_pairs && a.n_sched == b.n_sched &&
           a.reserve == b.reserve && a.truncated == b.truncated && a.n_trunc == b.n_trunc && a.n_groups == b.n_groups &&
           a.n_blend_rows == b.n_blend_rows && a.n_cpen == b.n_cpen;
}

int main() {
    // ---- NULL or all-off records: the blended plan there was before, form by form, with and without a map
    for (int top_k : {1, 50}) {
        for (float pen : {1.0f, 1.3f}) {
            for (bool tr : {false, true}) {
                for (bool grouped : {false, true}) {
                    Req plain(4, top_k), off(4, top_k);
                    plain.rows[1].repetition_penalty = off.rows[1].repetition_penalty = pen;
                    if (tr) {
                        plain.trunc.assign(4, mgea_row_truncation{0.05f, 0, 0, 0});
                        off.trunc = plain.trunc;
                    }
                    if (grouped) {
                        plain.blend.assign(4, mgea_row_blend{-1, 0.f});
                        plain.blend[0] = plain.blend[2] = mgea_row_blend{0, 0.5f};
                        off.blend = plain.blend;
                    }
                    off.with_cpen();
                    off.cpen[2].window = 17;      // a window alone switches nothing on
                    off.cpen[3].presence = -0.f;  // -0 is 0
                    const GenPlan a = planned(plain), b = planned(off), c = planned(off, kNoMap), d = planned(plain, kNoMap);
                    CHECK(same_plan(a, b) && same_plan(a, c) && same_plan(a, d) && !b.kind.class_penalized && b.n_cpen == 0);
                    CHECK(a.kind.blended == grouped);
                }
            }
        }
    }
    // ---- a row that is on => the flag, the count, never GREEDY
    {
        Req r(5, 1);   // all-greedy rows run as top_k == 1 records of the SAMPLED form
        r.on(3, 0.5f, 0.f, 4);
        GenPlan p = planned(r);
        CHECK(p.kind.class_penalized && p.kind.form == StepForm::SAMPLED && p.n_cpen == 1 && !p.kind.blended && !p.kind.guided && !p.kind.scored);
        r.on(0, 0.f, -2.f, 0);   // presence alone, negative, the whole history
        p = planned(r);
        CHECK(p.kind.class_penalized && p.n_cpen == 2);
        r.rows[0].repetition_penalty = 1.2f;
        p = planned(r);
        CHECK(p.kind.class_penalized && p.kind.form == StepForm::PENALIZED);
        r.trunc.assign(5, mgea_row_truncation{0, 0, 0, 0});
        r.trunc[4].min_p = 0.1f;
        r.rows[4].top_k = 50;
        p = planned(r);
        CHECK(p.kind.class_penalized && p.kind.truncated && p.kind.form == StepForm::BIASED);
        r.q.logprobs_out = g_lp;
        p = planned(r);
        CHECK(p.kind.class_penalized && p.kind.scored && p.kind.form == StepForm::BIASED);
        p = planned(r, kWin);
        CHECK(p.kind.class_penalized && p.kind.scored && p.kind.windowed);
    }
    {   // with a pair, a group and a schedule in one batch: every flag, every launch
        Req r(8, 1);
        r.guide.assign(8, mgea_row_guidance{-1, 0.f});
        r.guide[0] = {7, 1.5f};
        r.blend.assign(8, mgea_row_blend{-1, 0.f});
        r.blend[1] = {1, 0.6f};
        r.blend[2] = {1, 0.3f};
        r.blend[3] = {1, 0.1f};
        r.sched.assign(8, mgea_row_schedule{});
        for (auto& s : r.sched) s.n_segments = 1;
        r.sched[5].n_segments = 2;
        r.sched[5].threshold[0] = 4;
        r.q.n_seg_max = 2;
        r.on(0, 0.5f, 2.f, 4).on(1, 0.f, 1e4f, 4).on(5, -1e4f, 0.f, 4096);   // the bounds themselves are allowed
        const GenPlan p = planned(r);
        CHECK(p.kind.guided && p.kind.blended && p.kind.scheduled && p.kind.class_penalized && p.n_cpen == 3 && p.kind.form == StepForm::SAMPLED);
    }
    {   // a grammar row
        Req r(3, 50);
        const int32_t starts[3] = {0, -1, 1};
        r.q.start_states = starts;
        GenLimits g = kTiny;
        g.gram_n_state = 2;
        r.on(2, 1.f, 0.f, 8);
        const GenPlan p = planned(r, g);
        CHECK(p.grammar && p.kind.form == StepForm::GRAMMAR && p.kind.class_penalized);
    }
    // ---- the step-graph key: class_penalized is part of it, the values, windows and rows are not
    {
        Req a(4, 50), b(4, 50), c(4, 50);
        a.on(0, 0.5f, 0.f, 4);
        c.on(1, -3.f, 1.f, 0).on(3, 0.f, 7.f, 100);
        const GenPlan pa = planned(a), pb = planned(b), pc = planned(c);
        CHECK(pa.kind.form == pb.kind.form && !(pa.kind == pb.kind) && pa.kind == pc.kind);
        StepKind k = pb.kind;
        k.class_penalized = true;
        CHECK(k == pa.kind);
        const StepKind six{StepForm::SAMPLED, false, false, false, false, false, false};   // the aggregate the older tests write
        CHECK(!six.class_penalized && six == pb.kind);
    }
    // ---- the refusals, naming the row
    for (float v : {NAN, INFINITY, -INFINITY, 1.0001e4f, -2e4f, strtof("1e39", nullptr)}) {
        Req r(4, 50);
        r.on(1, 0.5f, 0.f, 4).on(2, v, 0.f, 4);
        CHECK(refused(r, "row 2", "frequency"));
        Req s(4, 50);
        s.on(3, 0.5f, v, 4);
        CHECK(refused(s, "row 3", "presence"));
    }
    for (int w : {-1, 4097, 1 << 30}) {
        Req r(4, 50);
        r.on(2, 0.5f, 0.f, w);
        CHECK(refused(r, "row 2", "window"));
        Req off(4, 50);   // a record that is off is checked too
        off.on(1, 0.f, 0.f, w);
        CHECK(refused(off, "row 1", "window"));
    }
    {
        Req r(4, 50);
        r.on(0, 0.5f, 0.f, 4);
        r.cpen[3].reserved = 1;
        CHECK(refused(r, "row 3", "reserved"));
    }
    {   // the first bad row is the one named
        Req r(4, 50);
        r.on(1, NAN, 0.f, 4).on(2, 0.f, NAN, 4);
        CHECK(refused(r, "row 1", "frequency"));
    }
    {   // window 0 counts the whole history: at most 4096 steps
        Req r(4, 50);
        r.q.n_steps = 4097;
        r.on(1, 0.5f, 0.f, 0);
        CHECK(refused(r, "row 1", "needs a window", kWin));
        r.on(1, 0.5f, 0.f, 4096);
        CHECK(planned(r, kWin).kind.class_penalized);
        r.on(1, 0.f, 0.f, 0);   // off: nothing to count
        CHECK(!planned(r, kWin).kind.class_penalized);
        r.q.n_steps = 4096;
        r.on(1, 0.5f, 0.f, 0);
        CHECK(planned(r, kWin).kind.class_penalized);
    }
    {   // a row that is on needs a map
        Req r(4, 50);
        r.on(2, 0.f, 1.f, 4);
        CHECK(refused(r, "row 2", "no class map", kNoMap));
        CHECK(planned(r).n_cpen == 1);
    }
    {   // the check alone, as mgea_op_class_penalty calls it: no step count
        const mgea_row_class_penalty recs[2] = {{0.5f, 0.f, 0, 0}, {0.f, 0.f, 9, 0}};
        int n = -1;
        CHECK(check_row_class_penalty(recs, 2, -1, 3, "op_class_penalty", &n) == MGEA_OK && n == 1);
        CHECK(class_penalty_on(recs[0]) && !class_penalty_on(recs[1]));
    }
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("class_penalty_plan ok\n");
    return 0;
}
