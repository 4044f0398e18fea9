// generate() behind the C ABI: plan (gen_plan.h), prefill, stage, run, finish over the engine of decoder.hip, and the entry points of
// the per-row features -- grammar, guidance, schedules, truncation, blends, class penalties, the KV window -- with their readers.
#include <cmath>

#include "decoder_handle.h"

using namespace mgea;

namespace {
// The buffers of a scheduled generation (dev_cond), big enough for `bytes` of store.  They are allocated, and regrown, by scheduled
// calls only; a regrow frees pointers the scheduled graphs hold, so it synchronises and drops those.
int ensure_cond(mgea_decoder* h, int64_t bytes, hipStream_t st) {
    if (h->cond.store && bytes <= h->cond.bytes) return MGEA_OK;
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying, a freed store still be read
    h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.scheduled; });
    DevGroup& g = h->dev_cond;
    g.release();
    h->pinned_cond.release();
    h->cond.bytes = 0;
    const size_t mb = (size_t)h->cfg.max_batch;
    if (g.alloc(&h->cond.store, (size_t)bytes) || h->cond.sched.allocate(g, h->pinned_cond, h->cfg.max_batch) ||
        g.alloc(&h->cond.cur_seg, mb * sizeof(int32_t)) || g.alloc(&h->cond.switches, 16) || g.alloc(&h->cond.meta, 16) ||
        g.alloc(&h->cond.len, mb * sizeof(int32_t))) {
        g.release();
        h->pinned_cond.release();
        set_error("decoder_generate_rows_scheduled: allocation of the conditioning store (%lld MB) failed", (long long)(bytes >> 20));
        return MGEA_ENOMEM;
    }
    h->cond.bytes = bytes;
    return MGEA_OK;
}

// ---- generate(): plan, prefill, stage, run, finish ------------------------------------------------------------------------------
// do_generate runs a GenRequest (gen_plan.h) in five phases, each a function of the request and its plan; the caller holds h->mu.

// A guidance shadow row runs on its conditional row's inputs -- same inputs, same id --, a non-leader member of a blend group on its
// leader's: src[u] is that row (mirror_sources, gen_plan.h), and this is the one place that hands them over.
// `part` names what the caller has just filled for the callers' rows:
//   PRESENCE  the seeded bitmaps: a pair's set is the conditional prompt plus the generated ids, and both tails add the same ids
//   RECORDS   the stages of the mirrored tables of `tabs` (rowtable.h): the sampler record -- seed, Philox stream, budget and all --,
//             the grammar start state, the truncation and class-penalty records (the rows are fed the same ids: the same counts)
//   BIAS      the engine's bias rows: the shadow adds its conditional row's vector (its record says bias_on as that one's does)
//   FORCED    the engine's forced-id rows: the shadow is told the ids its conditional row is told
enum class Mirror { PRESENCE, RECORDS, BIAS, FORCED };
int mirror_shadow_rows(mgea_decoder* h, const GenRequest& q, const GenPlan& p, const std::vector<int>& src, Mirror part, hipStream_t st,
                       const std::vector<RowTableBase*>* tabs = nullptr) {
    // the three device parts are rows of one matrix each: its base, its row stride and the bytes handed over
    const mgea_decoder::Hist hi = h->hist(p.kind.windowed);
    const size_t V = (size_t)h->cfg.vocab * sizeof(float), pw = (size_t)presence_words(h->cfg.vocab) * sizeof(uint32_t);
    char* base = reinterpret_cast<char*>(part == Mirror::PRESENCE ? (void*)h->presence : part == Mirror::BIAS ? (void*)h->bias : (void*)hi.forced);
    const size_t stride = part == Mirror::PRESENCE ? pw : part == Mirror::BIAS ? V : (size_t)hi.stride * sizeof(int32_t);
    const size_t bytes = part == Mirror::FORCED ? (size_t)q.n_steps * sizeof(int32_t) : stride;
    for (int u = 0; u < (int)src.size(); ++u) {   // (src is empty where the call has neither pairs nor groups)
        const int b = src[(size_t)u];
        if (b < 0 || (part == Mirror::BIAS && !h->samp.s()[b].bias_on)) continue;
        if (part != Mirror::RECORDS) {
            MGEA_CHECK_HIP(hipMemcpyAsync(base + (size_t)u * stride, base + (size_t)b * stride, bytes, hipMemcpyDeviceToDevice, st));
            continue;
        }
        for (RowTableBase* t : *tabs)
            if (t->mirrored) t->copy_row(u, b);
    }
    return MGEA_OK;
}

// Prefill: for a scheduled call the variants' prefills and gathers, then the generation's own reset and prefill (logits dropped,
// api_cache.py:163) and the presence seed.  Leaves the cache, cur_ids and the host mirror as the first step reads them.
int gen_prefill(mgea_decoder* h, const GenRequest& q, const GenPlan& p, const std::vector<int>& src, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = q.B, Tp = q.Tp;
    const bool windowed = p.kind.windowed;
    // positions [0, lens) of the prefill that has just finished -> segment sg of the conditioning store (the pool as the attention sees
    // it: the allocation rule where the prefill's pages follow it, the table otherwise)
    auto gather = [&](int sg) {
        return launch_cond_gather(kv_view(h), c.n_layer, h->page_table, h->max_pages, q.lens, Tp, h->cond.store, sg, q.n_seg_max, Tp, h->cond.meta,
                                  h->cond.len, B, st);
    };
    if (p.kind.scheduled) {
        // The variants behind the first, last to first: each a reset and a prefill of the B prompts with the call's own B, Tp and lens --
        // the kernels the generation's own prefill takes, so the gathered K | V are bit for bit what a generation from that variant caches.
        MGEA_TRY(ensure_cond(h, cond_store_bytes(h->kv, c.n_layer, q.n_seg_max, B, Tp), st));
        for (int sg = q.n_seg_max - 1; sg >= 1; --sg) {
            MGEA_TRY(do_reset(h, B, p.reserve, st));
            if (windowed) h->kv.arith_batch = 0;
            MGEA_TRY(do_forward(h, q.prompt_ids + (size_t)sg * B * Tp, q.lens, B, Tp, nullptr, st));
            MGEA_TRY(gather(sg));
        }
    }
    MGEA_TRY(do_reset(h, B, p.reserve, st));
    if (windowed) {   // the rotation breaks the allocation rule: every page id of the call comes from the table, the prefill's included
        h->kv.arith_batch = 0;
        MGEA_CHECK_HIP(hipMemsetAsync(h->win.evict, 0, (size_t)c.max_batch * sizeof(int32_t), st));
    }
    if (causal(c)) {
        // Every token is fed once: the prefill takes the prompts without their last tokens (same ids, width and stride, lengths - 1), and
        // the first step feeds the last token at position len - 1.  A prompt of one token prefills nothing.
        MGEA_TRY(launch_lens_minus_one(q.lens, h->lens_m1, Tp, B, st));
        if (Tp > 1) MGEA_TRY(do_forward(h, q.prompt_ids, h->lens_m1, B, Tp, nullptr, st));
        MGEA_TRY(launch_take_last(q.prompt_ids, q.lens, h->cur_ids, B, Tp, st));
    } else {
        MGEA_TRY(do_forward(h, q.prompt_ids, q.lens, B, Tp, nullptr, st));
    }
    if (p.kind.scheduled) {   // the generation's own prefill is segment 0; every row starts there
        MGEA_TRY(gather(0));
        MGEA_CHECK_HIP(hipMemsetAsync(h->cond.cur_seg, 0, (size_t)c.max_batch * sizeof(int32_t), st));
        MGEA_CHECK_HIP(hipMemsetAsync(h->cond.switches, 0, 16, st));
    }
    h->win.dirty = windowed;
    if (form_has_presence(p.kind.form)) {   // every row's set starts as its real prompt tokens
        MGEA_TRY(launch_presence_seed(q.prompt_ids, q.lens, B, Tp, c.vocab, h->presence, st));
        MGEA_TRY(mirror_shadow_rows(h, q, p, src, Mirror::PRESENCE, st));
    }
    return MGEA_OK;
}

// Stage: everything the steps read besides the cache goes into engine memory, stream-ordered and without a host sync -- the rows'
// records, bias vectors, grammar states, pairs, schedules and forced ids.  The captured graphs point at the engine's buffers, so one
// graph serves every step of every request.
int gen_stage(mgea_decoder* h, const GenRequest& q, const GenPlan& p, const std::vector<int>& src, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = q.B;
    if (q.rows) {
        // the tables' pinned stages are free once the previous call's uploads out of them have run
        MGEA_CHECK_HIP(hipEventSynchronize(h->stage_free.ev));
        // Fill: every table the plan switches on, from the request's records
        std::vector<RowTableBase*> tabs{&h->samp};
        auto stage = [&](auto& table, bool on, auto value_of) {
            if (!on) return;
            for (int b = 0; b < B; ++b) table.set(b, value_of(b));
            tabs.push_back(&table);
        };
        build_row_records(q.rows, q.lrows, B, q.n_steps, h->samp.s());
        stage(h->gram.state, p.grammar, [&](int b) { return q.start_states[b]; });
        stage(h->trunc.rec, p.truncated, [&](int b) { return q.trunc[b]; });
        stage(h->cpen.rec, p.kind.class_penalized, [&](int b) { return q.cpen[b]; });
        stage(h->guide.partner, p.kind.guided, [&](int b) { return q.guide[b].shadow_row; });
        stage(h->guide.scale, p.kind.guided, [&](int b) { return q.guide[b].shadow_row >= 0 ? q.guide[b].scale : 0.f; });
        stage(h->blend.leader, p.kind.blended, [&](int b) { return q.blend[b].leader; });
        stage(h->blend.weight, p.kind.blended, [&](int b) { return q.blend[b].leader >= 0 ? q.blend[b].weight : 0.f; });
        stage(h->cond.sched, p.kind.scheduled, [&](int b) { return q.sched[b]; });
        // Mirror (the tables that hold a row's inputs), then the rows' bias vectors -> their rows of the engine's buffer; upload
        MGEA_TRY(mirror_shadow_rows(h, q, p, src, Mirror::RECORDS, st, &tabs));
        for (int b = 0; p.biased && b < B; ++b)
            if (q.lrows[b].bias_dev)
                MGEA_CHECK_HIP(hipMemcpyAsync(h->bias + (size_t)b * c.vocab, q.lrows[b].bias_dev, (size_t)c.vocab * sizeof(float),
                                              hipMemcpyDeviceToDevice, st));
        if (p.biased) MGEA_TRY(mirror_shadow_rows(h, q, p, src, Mirror::BIAS, st));
        for (RowTableBase* t : tabs) MGEA_TRY(t->upload(B, st));
        MGEA_CHECK_HIP(hipEventRecord(h->stage_free.ev, st));
        if (p.capped) MGEA_TRY(launch_clamp_budgets(h->samp.d(), q.lens, q.Tp, B, p.reserve, st));
    } else {
        MGEA_TRY(launch_fill_sampler_params(h->samp.d(), sampler_params(*q.sampler, q.penalty), B, st));
    }
    if (p.kind.scored) {   // the engine's forced-id rows: -1 everywhere, then the caller's [B, n_steps] matrix (steps beyond it stay free)
        const mgea_decoder::Hist hi = h->hist(p.kind.windowed);
        const size_t hs = (size_t)hi.stride;
        MGEA_CHECK_HIP(hipMemsetAsync(hi.forced, 0xff, (size_t)B * hs * sizeof(int32_t), st));
        if (q.forced)
            MGEA_CHECK_HIP(hipMemcpy2DAsync(hi.forced, hs * sizeof(int32_t), q.forced, (size_t)q.n_steps * sizeof(int32_t),
                                            (size_t)q.n_steps * sizeof(int32_t), B, hipMemcpyDeviceToDevice, st));
        MGEA_TRY(mirror_shadow_rows(h, q, p, src, Mirror::FORCED, st));
    }
    return MGEA_OK;
}

// Run: the qkv0 table and the step graphs of this batch size and kind, the first step's embedding, then the launches -- with a poll
// every 16 steps where some row can finish early.  *launched = the steps that ran.
int gen_run(mgea_decoder* h, const GenRequest& q, const GenPlan& p, hipStream_t st, int* launched_out) {
    const int B = q.B, n_steps = q.n_steps;
    if (const int path = qkv0_path(h, B); path >= 0) MGEA_TRY(ensure_qkv0(h, path, st));   // before any capture of this batch size
    hipGraphExec_t gexec = nullptr, gexec_k = nullptr;
    if (!h->no_graph) MGEA_TRY(step_graph(h, B, p.kind, 1, st, &gexec));
    // several steps per graph launch (switch decoder_graph_steps, a divisor of 16 so that the EOS poll below keeps its rhythm)
    int K = h->no_graph || h->prof_stride > 0 ? 1 : tune(TUNE_DECODER_GRAPH_STEPS);
    if (K != 2 && K != 4 && K != 8 && K != 16) K = 1;
    if (K > 1 && n_steps >= K) MGEA_TRY(step_graph(h, B, p.kind, K, st, &gexec_k));
    MGEA_TRY(prime_gen(h, B, st));   // x <- embedding of the re-fed last prompt token (api_cache.py:167)
    int launched = 0;
    int32_t host_done = 0;
    while (launched < n_steps) {
        const int i = launched;
        if (h->prof_stride > 0 && (i % h->prof_stride) == h->prof_stride / 2) {
            h->prof_now = true;  // this step runs eagerly with HIP events around every launch
            const int rc = enqueue_gen_step(h, B, p.kind, st);
            h->prof_now = false;
            MGEA_TRY(rc);
            ++launched;
        } else if (h->no_graph) {
            MGEA_TRY(enqueue_gen_step(h, B, p.kind, st));
            ++launched;
        } else if (gexec_k && i % K == 0 && i + K <= n_steps) {
            MGEA_CHECK_HIP(hipGraphLaunch(gexec_k, st));
            launched += K;
        } else {
            MGEA_CHECK_HIP(hipGraphLaunch(gexec, st));
            ++launched;
        }
        if (p.may_stop_early && (launched % 16) == 0) {  // stop once every row has drawn EOS (api_cache.py:181) or spent its budget
            MGEA_CHECK_HIP(hipMemcpyAsync(&host_done, h->n_done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            MGEA_CHECK_HIP(hipStreamSynchronize(st));
            if (host_done >= B) break;
        }
    }
    if (p.capped) MGEA_TRY(launch_unpark_rows(h->done, h->ctx_len, B, st));
    h->host_max_len += launched;
    *launched_out = launched;
    return MGEA_OK;
}

// Finish: the steps that ran, from the histories into the caller's matrices; steps that never ran are 0 (log-probabilities) and -1 (ids)
int gen_finish(mgea_decoder* h, const GenRequest& q, const GenPlan& p, int launched, hipStream_t st) {
    const int B = q.B, n_steps = q.n_steps;
    const mgea_decoder::Hist hi = h->hist(p.kind.windowed);
    if (p.kind.scored) {
        float* outs[2] = {q.logprobs_out, q.choice_out};
        const float* hist[2] = {hi.lp, hi.ch};
        for (int i = 0; i < 2; ++i) {
            if (!outs[i]) continue;
            MGEA_CHECK_HIP(hipMemsetAsync(outs[i], 0, (size_t)B * n_steps * sizeof(float), st));
            MGEA_CHECK_HIP(hipMemcpy2DAsync(outs[i], (size_t)n_steps * sizeof(float), hist[i], (size_t)hi.stride * sizeof(float),
                                            (size_t)launched * sizeof(float), B, hipMemcpyDeviceToDevice, st));
        }
    }
    MGEA_CHECK_HIP(hipMemsetAsync(q.ids_out, 0xff, (size_t)B * n_steps * sizeof(int32_t), st));
    MGEA_CHECK_HIP(hipMemcpy2DAsync(q.ids_out, (size_t)n_steps * sizeof(int32_t), hi.ids, (size_t)hi.stride * sizeof(int32_t),
                                    (size_t)launched * sizeof(int32_t), B, hipMemcpyDeviceToDevice, st));
    return MGEA_OK;
}

int do_generate(mgea_decoder* h, const GenRequest& q, hipStream_t st) {
    const auto& c = h->cfg;
    const GenLimits lim{c.vocab, c.max_batch, c.max_ctx, c.block_mode, h->win.S, h->win.R, h->win.max_steps, h->gram.n_state, h->cpen.n_class};
    GenPlan p;
    MGEA_TRY(plan_generation(q, lim, &p));
    // (the conditioning store's [0, len) contract would need its own treatment where the last prompt token is not cached)
    MGEA_REQUIRE(!(causal(h->cfg) && q.sched), MGEA_EINVAL, "decoder_generate_rows_scheduled: MGEA_POS_CAUSAL engines take no prompt schedules");
    std::vector<int> src;   // the rows that run on another row's inputs: empty where the call has neither pairs nor groups
    if (p.kind.guided || p.kind.blended) src = mirror_sources(p.kind.guided ? q.guide : nullptr, p.kind.blended ? q.blend : nullptr, q.B);
    mgea_decoder::LastGen last;
    h->last = last;   // a call that fails from here on reports nothing
    MGEA_TRY(gen_prefill(h, q, p, src, st));
    last.penalized = form_has_presence(p.kind.form);
    last.scheduled = p.kind.scheduled;
    h->last = last;
    if (q.n_steps == 0) return MGEA_OK;
    MGEA_TRY(gen_stage(h, q, p, src, st));
    int launched = 0;
    MGEA_TRY(gen_run(h, q, p, st, &launched));
    last.plan = p;
    last.launched = launched;
    h->last = last;
    return gen_finish(h, q, p, launched, st);
}

// mgea_decoder_generate and _penalized: the uniform form (penalty 1: none, exactly the unpenalized launch sequence)
int generate_uniform(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp, int32_t n_steps,
                     const mgea_sampler_config* s, float repetition_penalty, int32_t* ids_out_dev, void* stream) {
    MGEA_REQUIRE(h && s && prompt_ids_dev && ids_out_dev, MGEA_EINVAL, "decoder_generate: NULL argument");
    MGEA_REQUIRE(std::isfinite(repetition_penalty) && repetition_penalty > 0.f, MGEA_EINVAL,
                 "decoder_generate: repetition_penalty must be finite and > 0 (got %g)", (double)repetition_penalty);
    GenRequest q;
    q.prompt_ids = prompt_ids_dev; q.lens = lens_dev; q.B = B; q.Tp = Tp; q.n_steps = n_steps;
    q.sampler = s; q.penalty = repetition_penalty; q.ids_out = ids_out_dev;
    std::lock_guard<std::mutex> lk(h->mu);
    return do_generate(h, q, (hipStream_t)stream);
}

// The mgea_decoder_generate_rows* entry points: one request from everything any of them takes (NULL = absent, n_seg_max 1), then their
// one prologue.  who NULL: the entry points from _scheduled on, named after the last records they were given.  What the records alone
// decide is checked before the handle is looked at (plan_generation checks it again, with the sampler records).
int generate_rows(mgea_decoder* h, const char* who, bool needs_logprobs, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                  int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* lrows, const int32_t* start_states, const mgea_row_guidance* guide,
                  const mgea_row_schedule* sched, int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                  float* choice_logprobs_out_dev, const mgea_row_truncation* trunc, const mgea_row_blend* blend, const mgea_row_class_penalty* cpen,
                  void* stream) {
    GenRequest q;
    q.who = who     ? who
            : cpen  ? "decoder_generate_rows_class_penalized"
            : blend ? "decoder_generate_rows_blended"
            : trunc ? "decoder_generate_rows_truncated"
                    : "decoder_generate_rows_scheduled";
    q.prompt_ids = prompt_ids_dev; q.lens = lens_dev; q.B = B; q.Tp = Tp; q.n_steps = n_steps;
    q.rows = rows; q.lrows = lrows; q.ids_out = ids_out_dev;
    q.start_states = start_states; q.guide = guide; q.sched = sched; q.n_seg_max = n_seg_max; q.trunc = trunc; q.blend = blend; q.cpen = cpen;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    MGEA_REQUIRE(q.rows && q.prompt_ids && q.ids_out && (q.logprobs_out || !needs_logprobs), MGEA_EINVAL, "%s: NULL argument", q.who);
    if (q.lrows) {
        MGEA_REQUIRE(q.B > 0, MGEA_EINVAL, "%s: empty batch", q.who);
        MGEA_TRY(check_row_logits(q.lrows, q.B, q.n_steps, q.who));
    }
    MGEA_REQUIRE(h, MGEA_EINVAL, "%s: NULL argument", q.who);
    MGEA_REQUIRE(q.logprobs_out || (!q.forced && !q.choice_out), MGEA_EINVAL,
                 "%s: forced ids and choice log-probabilities need logprobs_out_dev", q.who);
    MGEA_REQUIRE(q.n_seg_max >= 1 && q.n_seg_max <= MGEA_SCHEDULE_MAX_SEGMENTS, MGEA_EINVAL, "%s: n_seg_max %d outside [1, %d]", q.who,
                 q.n_seg_max, MGEA_SCHEDULE_MAX_SEGMENTS);
    MGEA_REQUIRE(q.sched || q.n_seg_max == 1, MGEA_EINVAL, "%s: %d prompt variants but no schedules", q.who, q.n_seg_max);
    std::lock_guard<std::mutex> lk(h->mu);
    return do_generate(h, q, (hipStream_t)stream);
}

// The _info and stats readers: under the lock, `fill` writes the figures of the last generate() (LastGen and its plan) and of the handle
template <class Fill>
int read_info(mgea_decoder* h, const int64_t* out, const char* who, Fill fill) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "%s: NULL argument", who);
    std::lock_guard<std::mutex> lk(h->mu);
    fill(h->last);
    return MGEA_OK;
}

}  // namespace

extern "C" {

int mgea_decoder_generate(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B,
                          int32_t Tp, int32_t n_steps, const mgea_sampler_config* s, int32_t* ids_out_dev,
                          void* stream) {
    return generate_uniform(h, prompt_ids_dev, lens_dev, B, Tp, n_steps, s, 1.0f, ids_out_dev, stream);
}

int mgea_decoder_generate_penalized(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B,
                                    int32_t Tp, int32_t n_steps, const mgea_sampler_config* s, float repetition_penalty,
                                    int32_t* ids_out_dev, void* stream) {
    return generate_uniform(h, prompt_ids_dev, lens_dev, B, Tp, n_steps, s, repetition_penalty, ids_out_dev, stream);
}

int mgea_decoder_generate_rows(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                               int32_t n_steps, const mgea_row_sampler* rows, int32_t* ids_out_dev, void* stream) {
    return generate_rows(h, "decoder_generate_rows", false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, nullptr, nullptr, nullptr, nullptr, 1, nullptr,
                         ids_out_dev, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_biased(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      int32_t* ids_out_dev, void* stream) {
    return generate_rows(h, "decoder_generate_rows", false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, nullptr, nullptr, nullptr, 1, nullptr,
                         ids_out_dev, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_scored(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                      float* choice_logprobs_out_dev, void* stream) {
    return generate_rows(h, "decoder_generate_rows_scored", true, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, nullptr, nullptr, nullptr, 1, forced_ids_dev,
                         ids_out_dev, logprobs_out_dev, choice_logprobs_out_dev, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_grammar(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                       int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                       const int32_t* start_states, const int32_t* forced_ids_dev, int32_t* ids_out_dev,
                                       float* logprobs_out_dev, float* choice_logprobs_out_dev, void* stream) {
    return generate_rows(h, "decoder_generate_rows_grammar", false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, nullptr, nullptr, 1, forced_ids_dev,
                         ids_out_dev, logprobs_out_dev, choice_logprobs_out_dev, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_guided(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      const int32_t* start_states, const mgea_row_guidance* guide, const int32_t* forced_ids_dev,
                                      int32_t* ids_out_dev, float* logprobs_out_dev, float* choice_logprobs_out_dev, void* stream) {
    return generate_rows(h, "decoder_generate_rows_guided", false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, guide, nullptr, 1, forced_ids_dev,
                         ids_out_dev, logprobs_out_dev, choice_logprobs_out_dev, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_scheduled(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                         int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                         const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                         int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                         float* choice_logprobs_out_dev, void* stream) {
    return generate_rows(h, nullptr, false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, guide, sched, n_seg_max, forced_ids_dev, ids_out_dev,
                         logprobs_out_dev, choice_logprobs_out_dev, nullptr, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_truncated(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                         int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                         const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                         int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                         float* choice_logprobs_out_dev, const mgea_row_truncation* trunc, void* stream) {
    return generate_rows(h, nullptr, false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, guide, sched, n_seg_max, forced_ids_dev, ids_out_dev,
                         logprobs_out_dev, choice_logprobs_out_dev, trunc, nullptr, nullptr, stream);
}

int mgea_decoder_generate_rows_blended(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                       int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                       const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                       int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                       float* choice_logprobs_out_dev, const mgea_row_truncation* trunc, const mgea_row_blend* blend,
                                       void* stream) {
    return generate_rows(h, nullptr, false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, guide, sched, n_seg_max, forced_ids_dev, ids_out_dev,
                         logprobs_out_dev, choice_logprobs_out_dev, trunc, blend, nullptr, stream);
}

int mgea_decoder_generate_rows_class_penalized(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                               int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                               const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                               int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev,
                                               float* logprobs_out_dev, float* choice_logprobs_out_dev, const mgea_row_truncation* trunc,
                                               const mgea_row_blend* blend, const mgea_row_class_penalty* cpen, void* stream) {
    return generate_rows(h, nullptr, false, prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, start_states, guide, sched, n_seg_max, forced_ids_dev, ids_out_dev,
                         logprobs_out_dev, choice_logprobs_out_dev, trunc, blend, cpen, stream);
}

int mgea_decoder_class_penalty_info(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_class_penalty_info", [&](const auto& l) {
        out[0] = h->cpen.n_class; out[1] = l.plan.n_cpen; out[2] = l.steps(l.plan.kind.class_penalized);
    });
}

int mgea_decoder_set_penalty_classes(mgea_decoder* h, const int32_t* class_of_host, int32_t n_class, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder_set_penalty_classes: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    const int V = h->cfg.vocab;
    auto clear = [&]() {
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.class_penalized; });
        h->dev_cpen.release();
        h->pinned_cpen.release();
        h->cpen.n_class = 0;
    };
    if (!class_of_host) {   // clear
        if (!h->cpen.class_of) return MGEA_OK;
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying, a freed map still be read
        clear();
        return MGEA_OK;
    }
    MGEA_REQUIRE(V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "decoder_set_penalty_classes: vocab %d exceeds the sampler's row (%d)", V,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(n_class >= 1 && n_class <= V, MGEA_EINVAL, "decoder_set_penalty_classes: n_class %d outside [1, %d]", n_class, V);
    for (int i = 0; i < V; ++i)
        MGEA_REQUIRE(class_of_host[i] >= -1 && class_of_host[i] < n_class, MGEA_EINVAL,
                     "decoder_set_penalty_classes: class_of[%d] = %d outside [-1, %d)", i, class_of_host[i], n_class);
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // the class-penalised graphs carry n_class; a replay may still be reading the old map
    h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.class_penalized; });
    if (!h->cpen.class_of) {
        if (h->dev_cpen.alloc(&h->cpen.class_of, (size_t)V * sizeof(int32_t)) ||
            h->cpen.rec.allocate(h->dev_cpen, h->pinned_cpen, h->cfg.max_batch)) {
            clear();
            set_error("decoder_set_penalty_classes: allocation of the class map failed");
            return MGEA_ENOMEM;
        }
        MGEA_CHECK_HIP(hipMemsetAsync(h->cpen.rec.d(), 0, (size_t)h->cfg.max_batch * sizeof(mgea_row_class_penalty), st));
    }
    MGEA_CHECK_HIP(hipMemcpyAsync(h->cpen.class_of, class_of_host, (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // the caller's map is host memory of unknown lifetime
    h->cpen.n_class = n_class;
    return MGEA_OK;
}

int mgea_decoder_blend_info(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_blend_info", [&](const auto& l) { out[0] = l.plan.n_groups; out[1] = l.plan.n_blend_rows; out[2] = l.steps(l.plan.kind.blended); });
}

int mgea_decoder_truncation_info(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_truncation_info", [&](const auto& l) { out[0] = l.steps(l.plan.truncated); out[1] = l.plan.truncated ? l.plan.n_trunc : 0; });
}

int mgea_decoder_set_grammar(mgea_decoder* h, const int32_t* class_of_host, const int32_t* next_host, int32_t n_state, int32_t n_class,
                             void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder_set_grammar: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    if (n_state == 0) {   // clear
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.form == StepForm::GRAMMAR; });
        h->gram.n_state = h->gram.n_class = 0;
        return MGEA_OK;
    }
    const int V = h->cfg.vocab;
    MGEA_REQUIRE(class_of_host && next_host, MGEA_EINVAL, "decoder_set_grammar: NULL table");
    MGEA_REQUIRE(n_class >= 1 && n_class <= MGEA_GRAMMAR_MAX_CLASSES, MGEA_EINVAL, "decoder_set_grammar: n_class %d outside [1, %d]", n_class,
                 MGEA_GRAMMAR_MAX_CLASSES);
    MGEA_REQUIRE(n_state >= 1 && n_state <= MGEA_GRAMMAR_MAX_STATES, MGEA_EINVAL, "decoder_set_grammar: n_state %d outside [1, %d]", n_state,
                 MGEA_GRAMMAR_MAX_STATES);
    MGEA_REQUIRE((int64_t)n_state * n_class <= MGEA_GRAMMAR_MAX_CELLS, MGEA_EINVAL, "decoder_set_grammar: n_state %d x n_class %d exceeds %d cells",
                 n_state, n_class, MGEA_GRAMMAR_MAX_CELLS);
    std::vector<char> populated((size_t)n_class, 0);
    for (int i = 0; i < V; ++i) {
        MGEA_REQUIRE(class_of_host[i] >= 0 && class_of_host[i] < n_class, MGEA_EINVAL, "decoder_set_grammar: class_of[%d] = %d outside [0, %d)", i,
                     class_of_host[i], n_class);
        populated[(size_t)class_of_host[i]] = 1;
    }
    for (int s = 0; s < n_state; ++s) {
        bool admits = false;
        for (int c = 0; c < n_class; ++c) {
            const int32_t v = next_host[(size_t)s * n_class + c];
            MGEA_REQUIRE(v >= -1 && v < n_state, MGEA_EINVAL, "decoder_set_grammar: next[%d][%d] = %d outside [-1, %d)", s, c, v, n_state);
            admits = admits || (v >= 0 && populated[(size_t)c]);
        }
        MGEA_REQUIRE(admits, MGEA_EINVAL, "decoder_set_grammar: state %d admits no class that has an id", s);
    }
    if (n_state != h->gram.n_state || n_class != h->gram.n_class) {
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.form == StepForm::GRAMMAR; });   // their kernel arguments carry the table's shape
    }
    MGEA_CHECK_HIP(hipMemcpyAsync(h->gram.class_of, class_of_host, (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipMemcpyAsync(h->gram.next, next_host, (size_t)n_state * n_class * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_TRY(launch_grammar_allow(h->gram.next, n_state, n_class, h->gram.allow, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // the caller's tables are host memory of unknown lifetime
    h->gram.n_state = n_state;
    h->gram.n_class = n_class;
    h->gram.uploads += 1;
    return MGEA_OK;
}

int mgea_decoder_schedule_info(mgea_decoder* h, int64_t* out, void* stream) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_schedule_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = out[1] = 0;
    if (!h->last.scheduled) return MGEA_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t n = 0;
    MGEA_CHECK_HIP(hipMemcpyAsync(&n, h->cond.switches, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    out[0] = h->last.steps(h->last.plan.kind.scheduled); out[1] = n;
    return MGEA_OK;
}

int mgea_decoder_segments(mgea_decoder* h, int32_t* out_dev, void* stream) {
    MGEA_REQUIRE(h && out_dev, MGEA_EINVAL, "decoder_segments: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_REQUIRE(h->last.scheduled && h->cur_batch > 0, MGEA_EINVAL, "decoder_segments: the last generate() was not scheduled");
    MGEA_CHECK_HIP(hipMemcpyAsync(out_dev, h->cond.cur_seg, (size_t)h->cur_batch * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_guidance_info(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_guidance_info", [&](const auto& l) { out[0] = l.plan.n_pairs; out[1] = l.steps(l.plan.kind.guided); });
}

int mgea_decoder_set_window(mgea_decoder* h, int32_t sink_pages, int32_t ring_pages, int32_t max_steps, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder_set_window: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    const auto& c = h->cfg;
    auto clear = [&]() {
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.windowed; });
        h->dev_win.release();
        h->win.hist.stride = 0;   // (its pointers: nulled by the group)
        h->win.S = h->win.R = h->win.max_steps = 0;
    };
    if (sink_pages == 0) {
        if (h->win.S == 0) return MGEA_OK;
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying, a freed history still be written
        clear();
        return MGEA_OK;
    }
    MGEA_REQUIRE(c.block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "decoder_set_window needs the KV-cache block mode");
    MGEA_REQUIRE(c.pos_mode == MGEA_POS_REFERENCE, MGEA_EINVAL,
                 "decoder_set_window: MGEA_POS_ABSOLUTE engines have no window (a step's position would be its cached length)");
    MGEA_REQUIRE(sink_pages >= 1, MGEA_EINVAL, "decoder_set_window: sink_pages %d must be >= 1 (0 clears the window)", sink_pages);
    MGEA_REQUIRE(ring_pages >= 2, MGEA_EINVAL,
                 "decoder_set_window: ring_pages %d must be >= 2 (one page would be evicted with the current token in it)", ring_pages);
    MGEA_REQUIRE(ring_pages <= WINDOW_MAX_RING, MGEA_EINVAL, "decoder_set_window: ring_pages %d exceeds %d", ring_pages, WINDOW_MAX_RING);
    MGEA_REQUIRE((int64_t)sink_pages + ring_pages <= c.max_ctx / MGEA_KV_PAGE_TOKENS, MGEA_EINVAL,
                 "decoder_set_window: sink_pages %d + ring_pages %d exceed the %d whole pages of max_ctx %d", sink_pages, ring_pages,
                 c.max_ctx / MGEA_KV_PAGE_TOKENS, c.max_ctx);
    MGEA_REQUIRE(max_steps >= 1 && max_steps <= MGEA_WINDOW_MAX_STEPS, MGEA_EINVAL, "decoder_set_window: max_steps %d outside [1, %d]",
                 max_steps, MGEA_WINDOW_MAX_STEPS);
    if (sink_pages == h->win.S && ring_pages == h->win.R && max_steps == h->win.max_steps) return MGEA_OK;
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    clear();   // the windowed graphs carry S, P and the histories' pointers
    const size_t nhist = (size_t)c.max_batch * (size_t)max_steps;
    DevGroup& g = h->dev_win;
    if (g.alloc(&h->win.hist.ids, nhist * sizeof(int32_t)) || g.alloc(&h->win.hist.forced, nhist * sizeof(int32_t)) ||
        g.alloc(&h->win.hist.lp, nhist * sizeof(float)) || g.alloc(&h->win.hist.ch, nhist * sizeof(float)) ||
        g.alloc(&h->win.evict, (size_t)c.max_batch * sizeof(int32_t))) {
        clear();
        set_error("decoder_set_window: allocation of the histories for max_steps %d failed", max_steps);
        return MGEA_ENOMEM;
    }
    MGEA_CHECK_HIP(hipMemsetAsync(h->win.evict, 0, (size_t)c.max_batch * sizeof(int32_t), st));
    h->win.hist.stride = max_steps;
    h->win.S = sink_pages; h->win.R = ring_pages; h->win.max_steps = max_steps;
    return MGEA_OK;
}

int mgea_decoder_window_info(mgea_decoder* h, int32_t* out, int32_t* evictions_out, void* stream) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_window_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->win.S; out[1] = h->win.R; out[2] = h->win.max_steps;
    if (evictions_out) {
        MGEA_REQUIRE(h->win.S > 0, MGEA_EINVAL, "decoder_window_info: no window is set");
        hipStream_t st = (hipStream_t)stream;
        const int B = h->cur_batch > 0 ? h->cur_batch : 0;
        MGEA_CHECK_HIP(hipMemcpyAsync(evictions_out, h->win.evict, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
    }
    return MGEA_OK;
}

int mgea_decoder_grammar_states(mgea_decoder* h, int32_t* out_dev, void* stream) {
    MGEA_REQUIRE(h && out_dev, MGEA_EINVAL, "decoder_grammar_states: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_CHECK_HIP(hipMemcpyAsync(out_dev, h->gram.state.d(), (size_t)(h->cur_batch > 0 ? h->cur_batch : 0) * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_grammar_info(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_grammar_info", [&](const auto& l) {
        out[0] = h->gram.n_state; out[1] = h->gram.n_class; out[2] = h->gram.uploads; out[3] = l.steps(l.plan.grammar);
    });
}

int mgea_decoder_presence(mgea_decoder* h, uint32_t* bits_out_dev, void* stream) {
    MGEA_REQUIRE(h && bits_out_dev, MGEA_EINVAL, "decoder_presence: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_REQUIRE(h->last.penalized && h->cur_batch > 0, MGEA_EINVAL, "decoder_presence: the last generate() applied no penalty");
    MGEA_CHECK_HIP(hipMemcpyAsync(bits_out_dev, h->presence, (size_t)h->cur_batch * presence_words(h->cfg.vocab) * sizeof(uint32_t),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_context_lengths(mgea_decoder* h, int32_t* lens_out_dev, void* stream) {
    MGEA_REQUIRE(h && lens_out_dev, MGEA_EINVAL, "context_lengths: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_CHECK_HIP(hipMemcpyAsync(lens_out_dev, h->ctx_len, (size_t)(h->cur_batch > 0 ? h->cur_batch : 0) * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_kv_pages(mgea_decoder* h, int32_t layer, void* pages_out_dev, int64_t pages_bytes, int32_t* page_table_out_dev,
                          int64_t* info_out, void* stream) {
    MGEA_REQUIRE(h && info_out, MGEA_EINVAL, "decoder_kv_pages: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const auto& c = h->cfg;
    MGEA_REQUIRE(h->kv.base, MGEA_EINVAL, "decoder_kv_pages needs the KV-cache block mode");
    MGEA_REQUIRE(layer >= 0 && layer < c.n_layer, MGEA_EINVAL, "decoder_kv_pages: layer %d of %d", layer, c.n_layer);
    const int64_t bytes = h->kv.layer_stride * (int64_t)h->kv.elt_bytes();
    info_out[0] = h->kv.n_pages; info_out[1] = h->max_pages; info_out[2] = h->kv.elt_bytes(); info_out[3] = bytes;
    if (!pages_out_dev && !page_table_out_dev) return MGEA_OK;   // the sizes only
    MGEA_REQUIRE(pages_out_dev && page_table_out_dev && pages_bytes >= bytes, MGEA_EINVAL, "decoder_kv_pages: a layer of pages is %lld bytes",
                 (long long)bytes);
    hipStream_t st = (hipStream_t)stream;
    MGEA_CHECK_HIP(hipMemcpyAsync(pages_out_dev, static_cast<const char*>(h->kv.base) + (int64_t)layer * bytes, (size_t)bytes,
                                  hipMemcpyDeviceToDevice, st));
    MGEA_CHECK_HIP(hipMemcpyAsync(page_table_out_dev, h->page_table, (size_t)c.max_batch * h->max_pages * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, st));
    return MGEA_OK;
}

int mgea_decoder_profile(mgea_decoder* h, int32_t stride) {
    MGEA_REQUIRE(h && stride >= 0, MGEA_EINVAL, "decoder_profile: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->prof_stride = stride;
    return MGEA_OK;
}

int mgea_decoder_profile_read(mgea_decoder* h, double* ms_by_class, int64_t* launches_by_class, int32_t n_classes) {
    MGEA_REQUIRE(h && ms_by_class && launches_by_class && n_classes >= PC_COUNT, MGEA_EINVAL, "decoder_profile_read: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_CHECK_HIP(hipDeviceSynchronize());
    for (int i = 0; i < n_classes; ++i) { ms_by_class[i] = 0.0; launches_by_class[i] = 0; }
    for (auto& r : h->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a.ev, r.b.ev) == hipSuccess) {
            ms_by_class[r.cls] += ms;
            launches_by_class[r.cls] += 1;
        }
    }
    h->prof.clear();
    return MGEA_OK;
}

int mgea_decoder_error_flags(mgea_decoder* h, int32_t* flags_out, void* stream) {
    MGEA_REQUIRE(h && flags_out, MGEA_EINVAL, "decoder_error_flags: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    int32_t v = 0;
    MGEA_CHECK_HIP(hipMemcpyAsync(&v, h->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    if (v) MGEA_CHECK_HIP(hipMemsetAsync(h->err_flag, 0, sizeof(int32_t), st));
    *flags_out = v;
    return MGEA_OK;
}

int mgea_decoder_qkv0_table_bytes(mgea_decoder* h, int64_t* bytes_out) {
    MGEA_REQUIRE(h && bytes_out, MGEA_EINVAL, "decoder_qkv0_table_bytes: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    int64_t n = 0;
    for (int p = 0; p < 2; ++p)
        if (h->qkv0_tab[p] && h->qkv0_ready[p]) n += (int64_t)h->cfg.vocab * 3 * h->cfg.d_model * (int64_t)sizeof(float);
    *bytes_out = n;
    return MGEA_OK;
}

int mgea_decoder_stats(mgea_decoder* h, int64_t* out) {
    return read_info(h, out, "decoder_stats", [&](const auto& l) {
        // the ABI's order (include/mgea.h), written down here and nowhere else
        out[0] = h->n.graph_nodes;
        out[1] = l.launched;
        out[2] = h->graphs.inserted();        // graph_instantiates: lifetime captures + instantiations
        out[3] = l.steps(l.plan.kind.scored);
        out[4] = (int64_t)h->graphs.size();   // graphs_cached
        out[5] = h->n.prefill16_forwards;
        out[6] = l.steps(l.plan.any_penalty);
        out[7] = l.steps(l.plan.biased);
    });
}

}  // extern "C"
