// plan_generation (csrc/gen_plan.h) and the rows' blend records (mgea_row_blend) on the CPU: blended => kind.blended and never the
// GREEDY form, both flags for a batch with a guidance pair and a group, the refusals with the row their message names, the capped call,
// NULL or all -1 records => the truncated plan there was before, the step-graph key, and mirror_sources, the row whose inputs each
// row of a batch with pairs and groups takes.  set_error is this file's own: it keeps the last message.  Run by tests/test_blend_host.py; exit status 0 and "blend_plan ok" = every check held.
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

// a tiny engine: 100 ids, 12 rows, 128 tokens of context, no window; the same with a window of 1 + 1 pages and 512 steps
const GenLimits kTiny{100, 12, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0};
const GenLimits kWin{100, 12, 128, MGEA_BLOCK_PRELN_GELU, 1, 1, 512, 0};

mgea_row_sampler row(int top_k, float penalty = 1.0f) { return mgea_row_sampler{1.0f, top_k, 0.f, penalty, -1, 0, 7u, 0u, 0u}; }
const mgea_row_blend kNone{-1, 0.f};
float g_lp[1];   // never dereferenced: a scored request is one with a logprobs_out

struct Req {
    std::vector<mgea_row_sampler> rows;
    std::vector<mgea_row_truncation> trunc;
    std::vector<mgea_row_guidance> guide;
    std::vector<mgea_row_schedule> sched;
    std::vector<mgea_row_blend> blend;
    GenRequest q;
    Req(int B, int top_k) : rows((size_t)B, row(top_k)) { q.B = B; q.Tp = 5; q.n_steps = 12; }
    Req& with_blend() { blend.assign(rows.size(), kNone); return *this; }
    // rows `members` become one group led by `leader`, each with weight w[i]
    Req& group(int leader, std::vector<int> members, std::vector<float> w) {
        if (blend.empty()) with_blend();
        for (size_t i = 0; i < members.size(); ++i) blend[(size_t)members[i]] = mgea_row_blend{leader, w[i]};
        return *this;
    }
    const GenRequest& get() {
        q.rows = rows.data();
        q.trunc = trunc.empty() ? nullptr : trunc.data();
        q.guide = guide.empty() ? nullptr : guide.data();
        q.sched = sched.empty() ? nullptr : sched.data();
        q.blend = blend.empty() ? nullptr : blend.data();
        return q;
    }
};

GenPlan planned(Req& r, const GenLimits& c = kTiny) {
    GenPlan p{};
    g_msg[0] = 0;
    CHECK(plan_generation(r.get(), c, &p) == MGEA_OK);
    return p;
}
bool refused(Req& r, const char* row_name, const char* what, int code = MGEA_EINVAL) {
    GenPlan p{};
    g_msg[0] = 0;
    return plan_generation(r.get(), kTiny, &p) == code && strstr(g_msg, row_name) != nullptr && strstr(g_msg, what) != nullptr;
}
bool same_plan(const GenPlan& a, const GenPlan& b) {
    return a.kind == b.kind && a.grammar == b.grammar && a.biased == b.biased && a.any_penalty == b.any_penalty &&
           a.may_stop_early == b.may_stop_early && a.capped == b.capped && a.n_pairs == b.n_pairs && a.n_sched == b.n_sched &&
           a.reserve == b.reserve && a.truncated == b.truncated && a.n_trunc == b.n_trunc && a.n_groups == b.n_groups &&
           a.n_blend_rows == b.n_blend_rows;
}

int main() {
    // ---- NULL or all -1 records: the truncated plan there was before, form by form
    for (int top_k : {1, 50}) {
        for (float pen : {1.0f, 1.3f}) {
            for (bool tr : {false, true}) {
                Req plain(4, top_k), off(4, top_k);
                plain.rows[1].repetition_penalty = off.rows[1].repetition_penalty = pen;
                if (tr) {
                    plain.trunc.assign(4, mgea_row_truncation{0.05f, 0, 0, 0});
                    off.trunc = plain.trunc;
                }
                off.with_blend();
                off.blend[2].weight = NAN;   // read only where leader >= 0
                const GenPlan a = planned(plain), b = planned(off);
                CHECK(same_plan(a, b) && !b.kind.blended && b.n_groups == 0 && b.n_blend_rows == 0);
            }
        }
    }
    // ---- blended => the flag, the counts, never GREEDY
    {
        Req r(5, 1);   // all-greedy rows run as top_k == 1 records of the SAMPLED form
        r.group(3, {1, 3}, {0.25f, 0.75f});
        GenPlan p = planned(r);
        CHECK(p.kind.blended && p.kind.form == StepForm::SAMPLED && p.n_groups == 1 && p.n_blend_rows == 2 && !p.kind.guided);
        r.rows[0].repetition_penalty = 1.2f;
        p = planned(r);
        CHECK(p.kind.blended && p.kind.form == StepForm::PENALIZED);
        r.trunc.assign(5, mgea_row_truncation{0, 0, 0, 0});
        r.trunc[4].min_p = 0.1f;
        r.rows[4].top_k = 50;
        p = planned(r);
        CHECK(p.kind.blended && p.kind.truncated && p.kind.form == StepForm::BIASED);
        r.q.logprobs_out = g_lp;
        p = planned(r);
        CHECK(p.kind.blended && p.kind.scored && p.kind.form == StepForm::BIASED);
    }
    {   // eight rows and a leader that is not the lowest; negative weights and a zero are fine
        Req r(12, 50);
        r.group(11, {1, 2, 4, 5, 6, 8, 9, 11}, {1.5f, -0.25f, -0.25f, 0.f, 0.5f, -0.5f, 0.25f, -0.25f});
        r.group(0, {0, 3}, {0.9995f, 0.f});   // within 1e-3 of 1
        const GenPlan p = planned(r);
        CHECK(p.kind.blended && p.n_groups == 2 && p.n_blend_rows == 10 && p.kind.form == StepForm::SAMPLED);
    }
    {   // a pair and a group on disjoint rows: both flags, both launches
        Req r(6, 1);
        r.guide.assign(6, mgea_row_guidance{-1, 0.f});
        r.guide[0] = {5, 1.5f};
        r.group(1, {1, 2, 3}, {0.6f, 0.3f, 0.1f});
        const GenPlan p = planned(r);
        CHECK(p.kind.guided && p.kind.blended && p.n_pairs == 1 && p.n_groups == 1 && p.n_blend_rows == 3 && p.kind.form == StepForm::SAMPLED);
    }
    // ---- the step-graph key: blended is part of it, the groups and weights are not
    {
        Req a(4, 50), b(4, 50), c(4, 50);
        a.group(0, {0, 1}, {0.5f, 0.5f});
        c.group(3, {1, 2, 3}, {2.f, -0.5f, -0.5f});
        const GenPlan pa = planned(a), pb = planned(b), pc = planned(c);
        CHECK(pa.kind.form == pb.kind.form && !(pa.kind == pb.kind) && pa.kind == pc.kind);
        StepKind k = pb.kind;
        k.blended = true;
        CHECK(k == pa.kind);
    }
    // ---- the refusals, naming the row
    {
        Req r(4, 50);
        r.group(0, {0, 1}, {0.5f, 0.5f});
        r.blend[2].leader = 4;
        CHECK(refused(r, "row 2", "leader 4 outside"));
        r.blend[2].leader = -2;
        CHECK(refused(r, "row 2", "leader -2 outside"));
    }
    {   // the named leader names nobody, or somebody else
        Req r(4, 50);
        r.with_blend();
        r.blend[1] = {2, 0.5f};
        r.blend[3] = {2, 0.5f};
        CHECK(refused(r, "row 1", "does not name itself"));
        r.blend[2] = {3, 0.5f};
        CHECK(refused(r, "row 1", "does not name itself"));
    }
    {   // a group of 1 and of 9
        Req r(4, 50);
        r.group(2, {2}, {1.0f});
        CHECK(refused(r, "row 2", "a group of 1 row"));
        Req n(12, 50);
        n.group(0, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {1.f, 0, 0, 0, 0, 0, 0, 0, 0});
        CHECK(refused(n, "row 8", "more than 8 rows"));
    }
    for (float w : {NAN, INFINITY, -INFINITY, strtof("1e39", nullptr)}) {   // 1e39 is inf as the float the record holds
        Req r(4, 50);
        r.group(1, {1, 3}, {0.5f, w});
        CHECK(refused(r, "row 3", "weight") && strstr(g_msg, "finite") != nullptr);
    }
    for (float w : {0.4f, 0.6f, 0.498f, 0.502f}) {   // sums 0.9, 1.1, 0.998, 1.002
        Req r(4, 50);
        r.group(1, {1, 3}, {0.5f, w});
        CHECK(refused(r, "row 1", "sum to"));
    }
    {   // a grouped row is neither side of a guidance pair
        Req r(6, 50);
        r.guide.assign(6, mgea_row_guidance{-1, 0.f});
        r.guide[0] = {5, 1.5f};
        r.group(0, {0, 1}, {0.5f, 0.5f});
        CHECK(refused(r, "row 0", "guidance pair"));
        r.with_blend().group(2, {2, 5}, {0.5f, 0.5f});
        CHECK(refused(r, "row 5", "guidance pair"));
    }
    {   // a grouped row has one segment
        Req r(4, 50);
        r.sched.assign(4, mgea_row_schedule{});
        for (auto& s : r.sched) s.n_segments = 1;
        r.sched[1].n_segments = 2;
        r.sched[1].threshold[0] = 4;
        r.q.n_seg_max = 2;
        r.group(0, {0, 2}, {0.5f, 0.5f});
        CHECK(planned(r).kind.blended && planned(r).kind.scheduled);   // a scheduled row outside the groups is fine
        r.group(0, {1}, {0.0f});
        CHECK(refused(r, "row 1", "segments"));
    }
    {   // a blended call is never capped; a window lifts the limit; the same call unblended is capped
        Req r(4, 50);
        r.q.n_steps = 124;   // 5 + 124 > 128
        r.group(0, {0, 1}, {0.5f, 0.5f});
        CHECK(refused(r, "decoder_generate_rows_blended", "never capped", MGEA_ECAPACITY));
        CHECK(planned(r, kWin).kind.blended && planned(r, kWin).kind.windowed);
        r.with_blend();
        CHECK(planned(r).capped);
        int g = -1, n = -1;
        CHECK(check_row_blend(r.blend.data(), 4, nullptr, nullptr, &g, &n) == MGEA_OK && g == 0 && n == 0);
    }
    // ---- mirror_sources: the row whose inputs each row takes -- a member its leader, a shadow its conditional row, -1 otherwise
    {
        using V = std::vector<int>;
        const mgea_row_guidance g0{-1, 0.f};
        Req r(6, 50);
        CHECK(mirror_sources(nullptr, nullptr, 6) == V(6, -1));                      // no pairs, no groups
        r.guide.assign(6, g0);
        r.with_blend();
        CHECK(mirror_sources(r.guide.data(), r.blend.data(), 6) == V(6, -1));        // records that name nobody
        r.guide[2] = {5, 1.5f};
        CHECK(mirror_sources(r.guide.data(), nullptr, 6) == (V{-1, -1, -1, -1, -1, 2}));   // one pair
        CHECK(mirror_sources(r.guide.data(), r.blend.data(), 6) == (V{-1, -1, -1, -1, -1, 2}));
        r.guide[2] = g0;
        r.guide[0] = {4, 1.5f};                                                      // a pair and a group in one batch of 6
        r.group(1, {1, 2, 5}, {0.6f, 0.3f, 0.1f});
        CHECK(planned(r).kind.guided && planned(r).kind.blended);
        CHECK(mirror_sources(r.guide.data(), r.blend.data(), 6) == (V{-1, -1, 1, -1, 0, 1}));
        CHECK(mirror_sources(nullptr, r.blend.data(), 6) == (V{-1, -1, 1, -1, -1, 1}));
    }
    {   // one group of MGEA_BLEND_MAX_ROWS rows whose leader is its last row: every other member points at it, a leader never at itself
        const int n = MGEA_BLEND_MAX_ROWS;
        Req r(n + 2, 50);
        std::vector<int> members;
        for (int i = 0; i < n; ++i) members.push_back(i + 1);
        r.group(n, members, std::vector<float>((size_t)n, 1.f / (float)n));
        CHECK(planned(r).n_blend_rows == n);
        const std::vector<int> src = mirror_sources(nullptr, r.blend.data(), n + 2);
        for (int u = 0; u < n + 2; ++u) CHECK(src[(size_t)u] == (u >= 1 && u < n ? n : -1));
        for (int u = 0; u < n + 2; ++u) CHECK(src[(size_t)u] != u);
    }
    {   // B = 64 with 32 pairs (the conditional rows and the shadows each in a scrambled order), and the same with two of the pairs
        // turned into groups: the list equals the double loop that stood in mirror_shadow_rows before it had one
        const int B = 64;
        std::vector<mgea_row_guidance> guide((size_t)B, mgea_row_guidance{-1, 0.f});
        std::vector<mgea_row_blend> blend((size_t)B, kNone);
        for (int i = 0; i < 32; ++i) guide[(size_t)((i * 7) % 32)] = {32 + (i * 11) % 32, 1.0f + 0.01f * (float)i};   // 7 and 11 are units mod 32
        for (int pass = 0; pass < 2; ++pass) {
            const GenLimits lim{100, 80, 128, MGEA_BLOCK_PRELN_GELU, 0, 0, 0, 0};
            Req r(B, 50);
            r.guide = guide;
            if (pass == 1) {   // two pairs less, their four rows in two groups
                r.guide[0] = r.guide[7] = mgea_row_guidance{-1, 0.f};
                r.with_blend();
                r.group(guide[0].shadow_row, {0, guide[0].shadow_row}, {0.5f, 0.5f});
                r.group(7, {7, guide[7].shadow_row}, {0.25f, 0.75f});
            }
            const GenPlan p = planned(r, lim);
            CHECK(p.n_pairs == (pass ? 30 : 32) && p.n_groups == (pass ? 2 : 0));
            const GenRequest& q = r.get();
            std::vector<int> want((size_t)B, -1);
            for (int u = 0; u < q.B; ++u) {   // the loop as it stood in mirror_shadow_rows
                int b = -1;
                if (p.kind.blended && q.blend[u].leader >= 0 && q.blend[u].leader != u) b = q.blend[u].leader;
                for (int c = 0; p.kind.guided && b < 0 && c < q.B; ++c)
                    if (q.guide[c].shadow_row == u) b = c;
                want[(size_t)u] = b;
            }
            const std::vector<int> got = mirror_sources(p.kind.guided ? q.guide : nullptr, p.kind.blended ? q.blend : nullptr, B);
            CHECK(got == want);
            int mirrored = 0;
            for (int u = 0; u < B; ++u) mirrored += got[(size_t)u] >= 0;
            CHECK(mirrored == 32);   // 32 shadows; 30 shadows and 2 members
        }
    }
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("blend_plan ok\n");
    return 0;
}
