// Decoder engine behind the C ABI: owns the paged KV pool, activation workspace and the captured
// hipGraph of one decode step.  Replaces GPTWithKV.forward / GPTBlock.forward / sample_kvcache
// (api_cache.py:51-74, 87-106, 159-184); weight names follow remap_state_dict (api_cache.py:118-134).
//
// Reference quirks reproduced on purpose: no attention mask anywhere (prefill is
// bidirectional), every call adds pos_emb[:T] so decode steps always use position row 0, the
// prefill logits are dropped and the first decode step re-feeds the last prompt token (which
// therefore sits in the cache twice).
#include <stdlib.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "devmem.h"
#include "hipres.h"

using namespace mgea;

namespace {
enum { T_TOK = 0, T_POS = 1, L_LN1W = 0, L_LN1B, L_INW, L_INB, L_OUTW, L_OUTB, L_LN2W, L_LN2B, L_FC1W, L_FC1B,
       L_FC2W, L_FC2B, L_COUNT };

int arena_layout(const mgea_decoder_config& c, std::vector<int64_t>* offs, int64_t* total) {
    const int64_t V = c.vocab, C = c.d_model, F = c.d_ff, L = c.seq_len;
    std::vector<int64_t> sizes;
    sizes.push_back(V * C);
    sizes.push_back(L * C);
    for (int i = 0; i < c.n_layer; ++i) {
        const int64_t s[L_COUNT] = {C, C, 3 * C * C, 3 * C, C * C, C, C, C, F * C, F, C * F, C};
        for (int j = 0; j < L_COUNT; ++j) sizes.push_back(s[j]);
    }
    sizes.push_back(V * C);
    sizes.push_back(V);
    int64_t o = 0;
    if (offs) offs->clear();
    for (int64_t s : sizes) {
        if (offs) offs->push_back(o);
        o += round_up(s, 64);
    }
    *total = o;
    return (int)sizes.size();
}

int validate(const mgea_decoder_config* c) {
    MGEA_REQUIRE(c, MGEA_EINVAL, "decoder config is NULL");
    MGEA_REQUIRE(c->vocab > 0 && c->seq_len > 0 && c->d_model > 0 && c->n_head > 0 && c->n_layer > 0 && c->d_ff > 0,
                 MGEA_EINVAL, "decoder config: non-positive dimension");
    MGEA_REQUIRE(c->d_model % c->n_head == 0, MGEA_EINVAL, "d_model %d not divisible by n_head %d", c->d_model, c->n_head);
    const int dh = c->d_model / c->n_head;
    // 96 = a 768-wide checkpoint under the reference's hard-coded 8 heads (api_cache.py:112)
    MGEA_REQUIRE(dh == 32 || dh == 64 || dh == 96, MGEA_EINVAL, "head_dim %d not supported (32, 64 or 96)", dh);
    MGEA_REQUIRE(c->d_model % 32 == 0 && c->d_ff % 32 == 0, MGEA_EINVAL, "d_model and d_ff must be multiples of 32");
    MGEA_REQUIRE(c->d_model <= 4096, MGEA_EINVAL, "d_model > 4096 not supported");
    MGEA_REQUIRE(c->max_batch > 0 && c->max_ctx > 0, MGEA_EINVAL, "max_batch / max_ctx must be positive");
    // the sampler keeps a row of logits in registers; refuse at create rather than at the first sampled generate()
    MGEA_REQUIRE(c->vocab <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "vocab %d exceeds the sampler's limit of %d", c->vocab,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(c->dtype == MGEA_DTYPE_F32 || c->dtype == MGEA_DTYPE_F16, MGEA_EINVAL,
                 "decoder dtype %d not supported (MGEA_DTYPE_F32 or MGEA_DTYPE_F16)", c->dtype);
    MGEA_REQUIRE(c->block_mode == MGEA_BLOCK_PRELN_GELU || c->block_mode == MGEA_BLOCK_POSTLN_RELU, MGEA_EINVAL, "bad block_mode");
    MGEA_REQUIRE(c->pos_mode != MGEA_POS_CAUSAL || c->block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL,
                 "MGEA_POS_CAUSAL needs the KV-cache block mode (the post-LN twin has no cache to extend)");
    if (c->dtype == MGEA_DTYPE_F16) {   // the fp16 mode lives on the fused decode path (tiled fp16 matrices, fp16 KV pages)
        MGEA_REQUIRE(c->block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "MGEA_DTYPE_F16 needs the KV-cache block mode");
        MGEA_REQUIRE((c->d_model % 128) == 0 && c->d_model >= 256 && c->d_model <= 1024, MGEA_EINVAL,
                     "MGEA_DTYPE_F16 needs d_model in 256..1024, a multiple of 128 (got %d)", c->d_model);
        MGEA_REQUIRE(dh == 32 || dh == 64, MGEA_EINVAL, "MGEA_DTYPE_F16 needs head_dim 32 or 64 (got %d)", dh);
    }
    return MGEA_OK;
}
// "use true positions": both modes that are not the reference's (every site that adds a position asks here)
bool true_positions(const mgea_decoder_config& c) { return c.pos_mode == MGEA_POS_ABSOLUTE || c.pos_mode == MGEA_POS_CAUSAL; }
bool causal(const mgea_decoder_config& c) { return c.pos_mode == MGEA_POS_CAUSAL; }
}  // namespace

struct mgea_decoder {
    mgea_decoder_config cfg{};
    const float* arena = nullptr;       // what every kernel reads: the caller's arena (f32) or arena_own (f16)
    // MGEA_DTYPE_F16: the model served is "the reference with its five projection-matrix kinds rounded to fp16".  arena_own is
    // a private fp32 copy of the caller's arena (arena_src) with exactly those tensors rounded, so that every path that reads
    // row-major fp32 weights (prefill beyond 512 rows, slab fallback) serves the SAME model as the fp16 tiles of the decode path.
    const float* arena_src = nullptr;
    float* arena_own = nullptr;
    int64_t arena_total = 0;
    bool f16 = false;
    std::vector<int64_t> off;
    int dh = 0;
    std::mutex mu;
    // Every device buffer below belongs to the group of its lifetime (devmem.h); a new one is allocated at the END of its group.
    DevGroup dev;            // handle state: mgea_decoder_create and build_tiled_weights, until destroy
    DevGroup dev_ws;         // the workspace: released and regrown by ensure_ws
    DevGroup dev_p16_rows;   // Prefill16's activations and tables, regrown with its row count (ensure_p16)
    DevGroup dev_p16_mats;   // Prefill16's matrices p16.w / p16.vec, kept across refresh_weights
    DevGroup dev_win;        // the KV window's histories and eviction counters: mgea_decoder_set_window, until the window changes
    DevGroup dev_cond;       // the conditioning store, the rows' schedules and segments: scheduled generations only (ensure_cond)
    DevGroup dev_cpen;       // the penalty class map and the rows' class-penalty records: mgea_decoder_set_penalty_classes, until it is cleared
    // The handle's other HIP resources, declared behind the device groups, so that they go first (members die in reverse order):
    // the graphs, the pinned staging arrays and the events, then the device memory.
    Event stage_free;        // recorded after the copy out of samp_stage / gram_stage: they may be rewritten once it has completed
    PinnedGroup pinned;      // samp_stage, gram_stage, guide_stage, cond_stage, trunc_stage, blend_stage
    PinnedGroup pinned_cpen; // cpen_stage: with dev_cpen

    // KV pool
    KvPool kv{};
    int pages_per_row_cap = 0;  // ceil(max_ctx / 64)
    int max_pages = 0;          // page-table row stride (== pages_per_row_cap)
    int32_t* page_table = nullptr;
    // per-row state
    int32_t *ctx_len = nullptr, *cur_ids = nullptr, *done = nullptr, *row_step = nullptr, *n_done = nullptr,
            *sampled = nullptr, *ids_hist = nullptr;
    int ids_hist_stride = 0;
    int32_t* lens_m1 = nullptr;   // [max_batch], MGEA_POS_CAUSAL engines only: the prompt lengths a generation prefills (gen_prefill)
    // host mirror
    int cur_batch = 0, reserved_len = 0, host_max_len = 0, host_min_len = 0;
    // workspace
    int64_t ws_tokens = 0;
    float *x = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *hbuf = nullptr, *slabs = nullptr,
          *logits = nullptr, *stats = nullptr, *pmax_val = nullptr;
    int32_t* pmax_idx = nullptr;
    int64_t pmax_cap = 0;        // entries of pmax_val / pmax_idx
    bool no_graph = false;       // MGEA_DECODER_NOGRAPH=1: launch every step eagerly (rocprofv3 --pmc runs)
    bool no_gemv = false;        // MGEA_DECODER_NOGEMV=1: keep the MFMA skinny GEMMs for batches of <= 2 rows too (A/B)
    bool force_unfused = false;  // MGEA_DECODER_UNFUSED=1: keep the 9-launch-per-layer path (A/B and fallback)
    int64_t slab_cap = 0;
    // Captured decode-step graphs, one per (batch, steps, StepKind): one per launch sequence.  Everything a step reads besides its
    // structure lives in device memory (per-row state, page table, presence bitmaps, and the rows' sampler records in samp_dev), so a
    // request with a new seed / temperature / top-k / top-p / EOS id / repetition penalty / budget -- or a batch whose rows differ in
    // them -- replays an existing graph: no capture, no instantiate.
    StepGraphs graphs;
    SamplerParams* samp_dev = nullptr;     // [max_batch] records, one per row (common.h)
    SamplerParams* samp_stage = nullptr;   // [max_batch] pinned host records of mgea_decoder_generate_rows, copied to samp_dev in stream order
    // repetition penalty: per row the set of ids it has seen (prompt + generated), [max_batch][presence_words(vocab)] (common.h);
    // seeded by a penalized generate() after its prefill, then updated by the kernel that commits each row's token
    uint32_t* presence = nullptr;
    // logit bias: [max_batch][vocab] fp32, row b = the vector row b adds to its logits when its record has bias_on.  A biased generate()
    // copies the rows' vectors here in stream order, so the captured graphs hold this pointer whatever the request's values.
    float* bias = nullptr;
    // scored generations (mgea_decoder_generate_rows_scored): forced [max_batch][ids_hist_stride] holds the ids the rows must take (-1 =
    // free), copied from the caller's matrix in stream order; lp_hist / ch_hist, next to ids_hist and with its stride, receive the raw and
    // the choice log-probability of every step; lp_step / ch_step [max_batch] carry one step's values from the sampler to advance_kernel
    // on the unfused path.  Engine-owned, so the scored graphs hold stable pointers whatever the request forces.
    int32_t* forced = nullptr;
    float *lp_hist = nullptr, *ch_hist = nullptr, *lp_step = nullptr, *ch_step = nullptr;
    // The KV window (mgea_decoder_set_window; the contract: include/mgea.h).  win_S > 0: every generation keeps P = win_S + win_R pages
    // per row -- the sink and a ring -- and each of its steps opens with the evict launch (kv_window.hip), so it may run win_max_steps
    // steps whatever max_ctx is.  Its id, forced-id and log-probability histories are therefore a second set, whist, with stride
    // win_max_steps, next to the rows' eviction counters win_evict [max_batch] in dev_win: allocated by set_window and by nothing else, so
    // an engine without a window allocates what it always did.  "Windowed" is part of the step-graph key; changing the window drops
    // those graphs alone.  win_dirty: a windowed generation has run since the last reset -- ctx_len counts cached tokens, the host
    // mirror (host_max_len) no longer says what the rows hold, and mgea_decoder_step / an extending forward are refused.
    int win_S = 0, win_R = 0, win_max_steps = 0;
    bool win_dirty = false;
    int32_t* win_evict = nullptr;
    struct Hist { int32_t* ids; int32_t* forced; float* lp; float* ch; int stride; };
    Hist whist{nullptr, nullptr, nullptr, nullptr, 0};
    Hist hist(bool windowed) const { return windowed ? whist : Hist{ids_hist, forced, lp_hist, ch_hist, ids_hist_stride}; }
    int32_t* err_flag = nullptr;   // sticky device flags (bit 0: a token id outside the vocabulary was clamped; bit 1: a forced id was banned by the grammar)
    // token grammar (mgea_decoder_set_grammar; GrammarArgs, common.h): one automaton per engine.  The tables live in buffers of their
    // largest size, allocated at create behind the other sampler buffers, so the GRAMMAR graphs hold stable pointers whatever table is
    // uploaded; the shape travels in the graphs' kernel arguments, so an upload of another shape drops those graphs.  gram_state
    // [max_batch]: the rows' states, filled from the call's start states (through the pinned gram_stage) before the first step.
    int32_t *gram_class = nullptr, *gram_next = nullptr, *gram_state = nullptr, *gram_stage = nullptr;
    uint32_t* gram_allow = nullptr;
    int gram_n_state = 0, gram_n_class = 0;
    int64_t gram_uploads = 0;
    // Classifier-free guidance (mgea_decoder_generate_rows_guided; guidance.hip): guide_partner [max_batch] holds the shadow row of every
    // conditional row (-1 elsewhere), guide_scale [max_batch] its scale.  Allocated at create behind the grammar's buffers and filled per
    // call through the pinned guide_stage ([max_batch] partners, then [max_batch] scales; free under stage_free like the records), so
    // the guided graphs hold stable pointers and a request with other pairs or scales replays them.
    int32_t* guide_partner = nullptr;
    float* guide_scale = nullptr;
    int32_t* guide_stage = nullptr;
    // Truncation (mgea_decoder_generate_rows_truncated; TruncArgs, common.h): trunc_dev [max_batch] holds the rows' min-p / typical-p /
    // epsilon / eta records.  Allocated at create behind the guidance vectors and filled per call through the pinned trunc_stage (free
    // under stage_free like the records), so the truncated graphs hold a stable pointer and a request with other values replays them.
    mgea_row_truncation *trunc_dev = nullptr, *trunc_stage = nullptr;
    // Emotion blends (mgea_decoder_generate_rows_blended; blend.hip): blend_leader [max_batch] holds every row's group leader (-1 = in no
    // group), blend_weight [max_batch] its weight.  Allocated at create behind the truncation records and filled per call through the
    // pinned blend_stage ([max_batch] leaders, then [max_batch] weights; free under stage_free like the records), so the blended graphs
    // hold stable pointers and a request with other groups or weights replays them.
    int32_t* blend_leader = nullptr;
    float* blend_weight = nullptr;
    int32_t* blend_stage = nullptr;
    // Windowed penalties over token classes (mgea_decoder_generate_rows_class_penalized; class_penalty.hip).  Everything here belongs to
    // dev_cpen / pinned_cpen and is allocated by mgea_decoder_set_penalty_classes, never by create: cpen_class [vocab] the map (values in
    // [-1, cpen_n_class)), cpen_dev [max_batch] the rows' records, filled per call through the pinned cpen_stage (free under stage_free
    // like the records), so the class-penalised graphs hold stable pointers and a request with other values or windows replays them.
    int32_t* cpen_class = nullptr;
    mgea_row_class_penalty *cpen_dev = nullptr, *cpen_stage = nullptr;
    int cpen_n_class = 0;
    // Emotion transitions (mgea_decoder_generate_rows_scheduled; recondition.hip).  Everything here belongs to dev_cond and is allocated by
    // the first scheduled call, never by create: cond_store holds the K | V of positions [0, len_b) of every prompt variant (cond_bytes
    // of it; a call that needs more synchronises, drops the scheduled graphs and regrows the whole group), cond_sched [max_batch] the
    // rows' records, cond_cur_seg [max_batch] their segments, cond_switches [1] the call's switch count, cond_meta [4] / cond_len
    // [max_batch] the store's layout words and the rows' prompt lengths (written by the gather kernel).  Records reach the device
    // through the pinned cond_stage, free under stage_free like the sampler records.
    void* cond_store = nullptr;
    int64_t cond_bytes = 0;
    mgea_row_schedule *cond_sched = nullptr, *cond_stage = nullptr;
    int32_t *cond_cur_seg = nullptr, *cond_switches = nullptr, *cond_meta = nullptr, *cond_len = nullptr;
    AttnSplit attn_split{};        // scratch of the split-context decode attention (small batches; attn_paged.hip)
    // The qkv0 table.  In MGEA_POS_REFERENCE mode every decode step adds pos_emb[0] (api_cache.py:99), so the input of layer 0's LN1 +
    // in-projection is tok_emb[id] + pos_emb[0]: its 3 C outputs q | k | v depend on the token id and the weights alone.  An f32 engine
    // computes them once for every id, with the step's own kernel family, into qkv0_tab [vocab][3 C] (a row's result does not depend on
    // the row-tile height the plan picks for a batch size: ensure_qkv0); the kernel that ends
    // a step and gathers the next embedding row gathers the table row too (common.h: embed_qkv0_row), and the layer-0 in-projection
    // launch leaves the captured step.  The rows of the MFMA kernel and of the <= 2-row dot-product kernel differ in their last bits
    // (LayerNorm folded / applied directly), so each decode path has a table of its own, [0] MFMA and [1] GEMV, built at the first
    // generation that takes the path; an engine that serves one path owns one table.
    bool qkv0_on = false;          // switch decoder_qkv0_table, latched at create
    float* qkv0_tab[2] = {nullptr, nullptr};
    bool qkv0_ready[2] = {false, false};   // false again after mgea_decoder_refresh_weights: rebuilt in place by the next generation
    bool qkv0_no_mem[2] = {false, false};  // the table could not be allocated: the path keeps the launch for the life of the handle (never
                                           // retried: the graphs of a batch size have one form)
    int32_t* qkv0_ids = nullptr;   // 0 .. vocab - 1, then 64 zeros: the ids and the ctx_len of the build launches
    // What the last generate() did, for the _info and stats entry points.  do_generate assigns it whole: zeroed once the call is
    // planned, with the two flags once its prefill is through, with the step counts once its steps have run.
    struct LastGen {
        bool penalized = false;   // it applied a penalty (or a bias): presence holds its rows
        bool scheduled = false;   // it was scheduled: cond_cur_seg / cond_switches hold its rows
        int64_t graph_replays = 0, scored_steps = 0, penalized_steps = 0, biased_steps = 0, gram_steps = 0, guide_pairs = 0, guide_steps = 0,
                sched_steps = 0, trunc_steps = 0, trunc_rows = 0, blend_groups = 0, blend_rows = 0, blend_steps = 0, cpen_rows = 0, cpen_steps = 0;
    } last;
    // what mgea_decoder_stats reports of the handle's lifetime, besides the graph cache's own two figures
    struct Counters { int64_t graph_nodes = 0, prefill16_forwards = 0; } n;
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg)
    int prof_stride = 0;  // 0 = off; n = time every n-th decode step of generate(), run eagerly
    bool prof_now = false;
    struct ProfRec { Event a, b; int cls; };
    std::vector<ProfRec> prof;   // unread records go with the handle

    const float* w(int idx) const { return arena + off[idx]; }
    const float* lw(int layer, int j) const { return arena + off[2 + layer * L_COUNT + j]; }
    const float* head_w() const { return arena + off[2 + cfg.n_layer * L_COUNT]; }
    const float* head_b() const { return arena + off[3 + cfg.n_layer * L_COUNT]; }
    // fragment-ordered copies of the five matrix kinds for the fused decode path (common.h: launch_tile_weights);
    // index 4 * layer + {0 in_proj, 1 out_proj, 2 fc1, 3 fc2}, then the head
    void* wt = nullptr;                 // fp32 fragments (f32) or _Float16 fragments (f16); offsets in elements
    std::vector<int64_t> wt_off;
    const float* wt_at(int64_t off) const {
        return reinterpret_cast<const float*>(static_cast<const char*>(wt) + off * (f16 ? 2 : 4));
    }
    // LayerNorm folded into in_proj (ln1) and fc1 (ln2): those two tiled matrices hold gamma * W, and lnv holds per layer
    // [c1 3C][c2 3C][c1 F][c2 F] (common.h: launch_ln_fold)
    float* lnv = nullptr;
    const float* qkv_c1(int l) const { return lnv + (int64_t)l * (6 * cfg.d_model + 2 * cfg.d_ff); }
    const float* qkv_c2(int l) const { return qkv_c1(l) + 3 * cfg.d_model; }
    const float* fc1_c1(int l) const { return qkv_c1(l) + 6 * cfg.d_model; }
    const float* fc1_c2(int l) const { return fc1_c1(l) + cfg.d_ff; }
    const float* tw(int layer, int j) const { return wt_at(wt_off[4 * layer + j]); }
    const float* head_tw() const { return wt_at(wt_off[4 * cfg.n_layer]); }

    // MGEA_DTYPE_F16, big-batch prefill on the f16 matrix cores (run_prefill16 below): fp16 activations, row-major fp16 matrices
    // (in_proj and fc1 with their LayerNorm's gamma folded in), statistics tables.  Allocated at the first such prefill.
    struct Prefill16 {
        int64_t rows = 0;
        void *x0 = nullptr, *x1 = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *w = nullptr;
        float *rowstat = nullptr, *stats_part = nullptr, *ident = nullptr, *vec = nullptr;
        int32_t* mask = nullptr;
        bool weights_ready = false;
        std::vector<int64_t> w_off;      // elements: per layer in_proj', out_proj, fc1', fc2; then the head
    } p16;
    const char* p16_w(int i) const { return static_cast<const char*>(p16.w) + p16.w_off[i] * 2; }
    float* p16_vec(int l, int which) const {   // 0 c1(in_proj) 1 c2(in_proj) 2 c1(fc1) 3 c2(fc1)
        float* base = p16.vec + (int64_t)l * (6 * cfg.d_model + 2 * cfg.d_ff);
        return which == 0 ? base : which == 1 ? base + 3 * cfg.d_model : which == 2 ? base + 6 * cfg.d_model : base + 6 * cfg.d_model + cfg.d_ff;
    }
};

namespace {

enum { PC_GEMM = 0, PC_ROWOP = 1, PC_ATTN_PAGED = 2, PC_ATTN_DENSE = 3, PC_SAMPLE = 4, PC_COUNT = 5 };

struct ProfScope {
    mgea_decoder* h;
    hipStream_t st;
    bool on;
    Event a, b;   // (half a pair, where the second create fails, goes with the scope)
    int cls;
    ProfScope(mgea_decoder* h_, int cls_, hipStream_t st_) : h(h_), st(st_), on(h_->prof_now), cls(cls_) {
        if (on) {
            on = hipEventCreate(&a.ev) == hipSuccess && hipEventCreate(&b.ev) == hipSuccess;
            if (on) (void)hipEventRecord(a.ev, st);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(b.ev, st);
            h->prof.push_back({std::move(a), std::move(b), cls});
        }
    }
};
#define PROF(cls, call)                \
    do {                               \
        ProfScope _ps(h, cls, st);     \
        MGEA_TRY(call);                \
    } while (0)

int64_t slab_need(const mgea_decoder_config& c, int M) {
    const int C = c.d_model, F = c.d_ff, V = c.vocab;
    const int shapes[5][2] = {{3 * C, C}, {C, C}, {F, C}, {C, F}, {V, C}};
    int64_t need = 0;
    const int Mh = M > 4096 ? 4096 : M;  // the head runs in row chunks of <= 4096
    for (int i = 0; i < 5; ++i) {
        const int m = (i == 4) ? Mh : M;
        const int64_t s = (int64_t)pick_split_k(m, shapes[i][0], shapes[i][1]) * slab_floats(m, shapes[i][0]);
        need = s > need ? s : need;
    }
    return need;
}

int ensure_ws(mgea_decoder* h, int64_t M) {
    M = round_up(M, 64);   // the k-tiled buffers of the fused path are whole 64-row groups
    if (M <= h->ws_tokens) return MGEA_OK;
    MGEA_CHECK_HIP(hipDeviceSynchronize());
    DevGroup& g = h->dev_ws;
    g.release();
    h->ws_tokens = h->slab_cap = 0;
    h->graphs.drop_all();  // captured pointers die with the old workspace
    const int C = h->cfg.d_model, F = h->cfg.d_ff;
    int64_t slab = slab_need(h->cfg, (int)M);
    const int64_t s64 = slab_need(h->cfg, 64);
    slab = slab > s64 ? slab : s64;
    auto floats = [&](float** field, int64_t n) {
        if (g.alloc(field, (size_t)n * sizeof(float)) == MGEA_OK) return true;
        set_error("decoder workspace: out of device memory (%lld floats)", (long long)n);
        return false;
    };
    const int64_t fr = M < MGEA_FUSED_MAX_ROWS ? M : MGEA_FUSED_MAX_ROWS;   // rows of the fused path
    const int64_t pcap = fr * ceil_div(h->cfg.vocab, 16);   // every head plan leaves at most one partial per 16 columns (checked in decode_gemm)
    const bool ok = floats(&h->x, M * C) && floats(&h->xn, M * C) && floats(&h->qkv, M * 3 * C) && floats(&h->att, M * C) &&
              floats(&h->hbuf, M * F) && floats(&h->slabs, slab) && floats(&h->logits, (int64_t)h->cfg.max_batch * h->cfg.vocab) &&
              floats(&h->stats, fr * (C / 16 + 1) * 2) && floats(&h->pmax_val, pcap);
    if (!ok || g.alloc(&h->pmax_idx, (size_t)pcap * sizeof(int32_t)) != MGEA_OK) {
        if (ok) set_error("decoder workspace: out of device memory");
        g.release();
        return MGEA_ENOMEM;
    }
    h->slab_cap = slab;
    h->pmax_cap = pcap;
    h->ws_tokens = M;
    return MGEA_OK;
}

// gemm + slab bookkeeping
int gemm(mgea_decoder* h, const float* A, int lda, const float* W, int M, int N, int K, int* S, hipStream_t st) {
    const int s = pick_split_k(M, N, K, h->slab_cap);
    MGEA_REQUIRE((int64_t)s * slab_floats(M, N) <= h->slab_cap, MGEA_ECAPACITY, "internal: slab workspace too small");
    ProfScope _ps(h, PC_GEMM, st);
    const int rc = launch_gemm_f32(A, lda, W, K, h->slabs, M, N, K, s, st);
    if (rc < 0) return rc;
    *S = rc;
    return MGEA_OK;
}

// The NL blocks over M = B*T rows.  use_cache_attn: attention over the paged cache (decode /
// extend); otherwise dense attention inside the qkv buffer (prefill with empty cache, twin mode).
// kv_only_last: the caller drops the logits (the prompt prefill of sample_kvcache, api_cache.py:163: `_, past = model(idx)`), so nothing
// reads the last block's output: once its K | V are in the cache the pass is over -- no attention, out-projection or MLP for that block.
int run_blocks(mgea_decoder* h, int B, int T, const int32_t* lens, bool use_cache_attn, bool scatter,
               hipStream_t st, bool kv_only_last = false) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, M = B * T;
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    for (int l = 0; l < c.n_layer; ++l) {
        int S = 1;
        const float* a_in = post ? h->x : h->xn;
        // big prefill: bias inside the QKV GEMM (qkv written once, no slab) and a scatter that only reads its K | V columns -- 0.5 GB less
        // traffic per block at [64, 1024].  Only where the slab form would not split K either (>= 256 tiles): the same sums.  (Rows past a
        // ragged prompt's length then hold the projection of their padding token instead of zeros; nothing reads them: the attention
        // masks them as keys by `lens` and their own outputs are ignored.)
        if (scatter && M > 64 && (int64_t)ceil_div(M, 128) * ceil_div(3 * C, 128) >= 256) {
            PROF(PC_GEMM, launch_gemm_f32_bias_act(a_in, C, h->lw(l, L_INW), C, h->lw(l, L_INB), h->qkv, 3 * C, M, 3 * C, C, ACT_NONE, st));
            PROF(PC_ROWOP, launch_qkv_scatter(h->qkv, 1, 0, 3 * C, nullptr, nullptr, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
        } else {
        MGEA_TRY(gemm(h, a_in, C, h->lw(l, L_INW), M, 3 * C, C, &S, st));
        KvPool kv = h->kv;
        if (!scatter) kv.base = nullptr;
        if (scatter) {
            PROF(PC_ROWOP, launch_qkv_scatter(h->slabs, S, slab_floats(M, 3 * C), (int)slab_ld(3 * C), h->lw(l, L_INB),
                                        h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
        } else {
            PROF(PC_ROWOP, launch_bias_act(h->slabs, S, slab_floats(M, 3 * C), (int)slab_ld(3 * C), h->lw(l, L_INB), h->qkv,
                                     3 * C, M, 3 * C, ACT_NONE, st));
        }
        }
        if (kv_only_last && scatter && l + 1 == c.n_layer) break;
        if (use_cache_attn) {
            PROF(PC_ATTN_PAGED, launch_attn_paged(h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, h->att, B, T,
                                       C, 0, st, &h->attn_split, causal(c)));
        } else {
            PROF(PC_ATTN_DENSE, launch_attn_dense(h->qkv, lens, nullptr, h->att, B, T, c.n_head, h->dh, 0, st, nullptr, causal(c)));
        }
        MGEA_TRY(gemm(h, h->att, C, h->lw(l, L_OUTW), M, C, C, &S, st));
        if (post) {
            PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_OUTB), h->x,
                                        nullptr, h->lw(l, L_LN1W), h->lw(l, L_LN1B), c.ln_eps, M, C, 1, st));
        } else {
            PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_OUTB), h->x,
                                        h->xn, h->lw(l, L_LN2W), h->lw(l, L_LN2B), c.ln_eps, M, C, 0, st));
        }
        if (gemm_direct_epilogue_ok((int)M, F)) {   // bias + activation inside the GEMM epilogue (no slab round trip)
            PROF(PC_GEMM, launch_gemm_f32_bias_act(post ? h->x : h->xn, C, h->lw(l, L_FC1W), C, h->lw(l, L_FC1B), h->hbuf, F, M, F,
                                                   C, post ? ACT_RELU : ACT_GELU, st));
        } else {
            MGEA_TRY(gemm(h, post ? h->x : h->xn, C, h->lw(l, L_FC1W), M, F, C, &S, st));
            PROF(PC_ROWOP, launch_bias_act(h->slabs, S, slab_floats(M, F), (int)slab_ld(F), h->lw(l, L_FC1B), h->hbuf, F, M, F,
                                     post ? ACT_RELU : ACT_GELU, st));
        }
        MGEA_TRY(gemm(h, h->hbuf, F, h->lw(l, L_FC2W), M, C, F, &S, st));
        if (post) {
            PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_FC2B), h->x,
                                        nullptr, h->lw(l, L_LN2W), h->lw(l, L_LN2B), c.ln_eps, M, C, 1, st));
        } else {
            const bool last = l + 1 == c.n_layer;
            PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_FC2B), h->x,
                                        h->xn, last ? nullptr : h->lw(l + 1, L_LN1W),
                                        last ? nullptr : h->lw(l + 1, L_LN1B), c.ln_eps, M, C, 0, st));
        }
    }
    return MGEA_OK;
}

// Fused path for M = B*T <= MGEA_FUSED_MAX_ROWS rows in the KV-cache block mode: 5 launches per layer
// (gemm_skinny.hip); x carries per-row LayerNorm partial statistics between kernels.
bool fused_geometry(const mgea_decoder_config& c) {
    return c.block_mode == MGEA_BLOCK_PRELN_GELU && (c.d_model % 128) == 0 && c.d_model >= 256 && c.d_model <= 1024;
}
bool fused_ok(const mgea_decoder* h, int M) {
    return fused_geometry(h->cfg) && M <= MGEA_FUSED_MAX_ROWS && M <= h->ws_tokens && !h->force_unfused && h->wt;
}

// single-token decode steps of <= 2 rows (the reference's serving case is B = 1): wave-level dot products on the
// row-major arena weights instead of 16 x 16 MFMA tiles (gemv_small.hip)
bool gemv_ok(const mgea_decoder* h, int M, int T, const int32_t* lens, bool use_cache_attn) {
    const auto& c = h->cfg;
    return !h->no_gemv && !h->f16 && T == 1 && !lens && use_cache_attn && gemv_shape_ok(M, c.d_model, c.d_model) &&
           gemv_shape_ok(M, c.d_model, c.d_ff);
}

// One decode GEMM -- g = 0 in_proj, 1 out_proj, 2 fc1, 3 fc2 of layer l, 4 the head -- on the weights of its family: the arena's
// row-major matrices with LayerNorm applied directly (gv: gemv_rows_kernel) or the tiled copies with LayerNorm folded in.
// `a` brings the activations and the epilogue's buffers; *plan (optional) receives what ran (the head's partial count).
int decode_gemm(mgea_decoder* h, int l, int g, SkinnyArgs a, bool gv, hipStream_t st, DecodeGemmPlan* plan = nullptr) {
    static const int kEpi[5] = {EPI_QKV, EPI_RES, EPI_ACT, EPI_RES, EPI_LOGITS};
    static const int kW[4] = {L_INW, L_OUTW, L_FC1W, L_FC2W}, kB[4] = {L_INB, L_OUTB, L_FC1B, L_FC2B};
    const bool ln = g == 0 || g == 2;
    const int lnw = g == 0 ? L_LN1W : L_LN2W, lnb = g == 0 ? L_LN1B : L_LN2B;
    a.w_f16 = h->f16;
    a.W = g == 4 ? (gv ? h->head_w() : h->head_tw()) : (gv ? h->lw(l, kW[g]) : h->tw(l, g));
    a.bias = g == 4 ? h->head_b() : h->lw(l, kB[g]);
    if (ln && gv) {
        a.ln_g = h->lw(l, lnw); a.ln_b = h->lw(l, lnb);
    } else if (ln) {   // LN(x) @ W^T + b = rstd * (x @ (gamma W)^T - mean * c1) + c2 (launch_ln_fold); fp16 tiles: gamma on A
        a.ln_c1 = g == 0 ? h->qkv_c1(l) : h->fc1_c1(l);
        a.bias = g == 0 ? h->qkv_c2(l) : h->fc1_c2(l);
        if (h->f16) a.ln_g = h->lw(l, lnw);
    }
    DecodeGemmPlan p;
    MGEA_TRY(plan_decode_gemm(kEpi[g], a, gv, &p));
    MGEA_REQUIRE(!a.pmax_val || (int64_t)a.M * p.n_partials <= h->pmax_cap, MGEA_EINVAL,
                 "decoder: %d rows x %d head partials exceed the workspace (%lld)", a.M, p.n_partials, (long long)h->pmax_cap);
    if (plan) *plan = p;
    return launch_decode_gemm(kEpi[g], p, a, st);
}

// qkv0_primed: h->qkv and layer 0's K | V page already hold this step's in-projection of layer 0 (the qkv0 table): that launch is skipped
int run_blocks_fused(mgea_decoder* h, int B, int T, const int32_t* lens, bool use_cache_attn, hipStream_t st,
                     bool kv_only_last = false, bool qkv0_primed = false) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, M = B * T;
    const bool gv = gemv_ok(h, M, T, lens, use_cache_attn);
    int n_part = 2, part_cnt = C / 2;  // the embedding kernel leaves the whole-row statistics as two equal halves
    for (int l = 0; l < c.n_layer; ++l) {
        // ln1 + in_proj + KV append
        SkinnyArgs a{};
        a.M = M; a.eps = c.ln_eps; a.A = h->x; a.lda = C; a.N = 3 * C; a.K = C;
        a.stats_in = h->stats; a.n_part = n_part; a.part_cnt = part_cnt;
        a.out = h->qkv; a.ldo = 3 * C;
        a.pool = h->kv; a.layer = l; a.page_table = h->page_table; a.max_pages = h->max_pages; a.ctx_len = h->ctx_len;
        if (!tune(TUNE_ATTN_ARITH_PAGES)) a.pool.arith_batch = 0;   // (as the attention: the switch sends every page id through the table)
        a.lens = lens; a.T = T; a.C = C;
        if (l > 0 || !qkv0_primed) PROF(PC_GEMM, decode_gemm(h, l, 0, a, gv, st));
        if (kv_only_last && l + 1 == c.n_layer) break;       // (run_blocks: the logits are dropped, the last block's K | V are appended)
        if (use_cache_attn) {
            PROF(PC_ATTN_PAGED, launch_attn_paged(h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, h->att, B, T, C, 1, st, &h->attn_split, causal(c)));
        } else {
            PROF(PC_ATTN_DENSE, launch_attn_dense(h->qkv, lens, nullptr, h->att, B, T, c.n_head, h->dh, 1, st, nullptr, causal(c)));
        }
        // out_proj + residual (+ stats for ln2)
        SkinnyArgs o{};
        o.M = M; o.eps = c.ln_eps; o.A = h->att; o.lda = C; o.N = C; o.K = C;
        o.out = h->x; o.ldo = C; o.stats_out = h->stats;
        PROF(PC_GEMM, decode_gemm(h, l, 1, o, gv, st));
        n_part = C / 16; part_cnt = 16;
        // ln2 + mlp.0 + GELU
        SkinnyArgs f{};
        f.M = M; f.eps = c.ln_eps; f.A = h->x; f.lda = C; f.N = F; f.K = C;
        f.stats_in = h->stats; f.n_part = n_part; f.part_cnt = part_cnt;
        f.out = h->hbuf; f.ldo = F; f.act = ACT_GELU;
        PROF(PC_GEMM, decode_gemm(h, l, 2, f, gv, st));
        // mlp.2 + residual (+ stats for the next ln1)
        SkinnyArgs r{};
        r.M = M; r.eps = c.ln_eps; r.A = h->hbuf; r.lda = F; r.N = C; r.K = F;
        r.out = h->x; r.ldo = C; r.stats_out = h->stats;
        PROF(PC_GEMM, decode_gemm(h, l, 3, r, gv, st));
    }
    return MGEA_OK;
}

// One decode step (T = 1) of the whole batch.
// kind: the step's launch sequence (StepKind, gen_plan.h); nothing below looks at a sampler setting to choose a kernel.
// pd: the rows' device records (generate()), or NULL and pv by value on every row (mgea_decoder_step).
// primed: x already holds the embedding (+ LN statistics) of cur_ids -- generate() keeps that invariant on the fused path by
// fusing the next step's embedding into this step's tail, so a replayed step is 32 launches.
struct StepCall {
    int B; StepKind kind;
    const SamplerParams* pd; SamplerParams pv;
    float* logits_out;   // optional
    bool primed;
    // primed steps only: the qkv0 table of the step's decode path -- layer 0's q | k | v arrive primed too (no in-projection launch for
    // layer 0) and the tail gathers them for the next step; NULL: the launch
    const float* qkv0 = nullptr;
    // where the head writes the logits row: the caller's buffer, the engine's `own` for the sampler, nowhere for the argmax tails
    float* head_out(float* own) const { return logits_out ? logits_out : (kind.form == StepForm::GREEDY ? nullptr : own); }
};

// What the kernel that embeds the next step's token works on; qkv0: the table of the step's path, or NULL (TailArgs, common.h)
TailArgs tail_args(const mgea_decoder* h, const StepState& s, const float* qkv0) {
    const auto& c = h->cfg;
    TailArgs t{s, h->w(T_TOK), h->w(T_POS), h->x, h->stats, c.d_model, c.vocab, c.seq_len, true_positions(c)};
    if (qkv0) {
        t.qkv0 = qkv0; t.qkv = h->qkv;
        t.pool = h->kv; t.page_table = h->page_table; t.max_pages = h->max_pages;
        if (!tune(TUNE_ATTN_ARITH_PAGES)) t.pool.arith_batch = 0;   // (as the attention: the switch sends every page id through the table)
    }
    return t;
}

// The tail of a step over the head's output.  GREEDY: the argmax of the head's n_partials partials per row (0: the ids are already in
// h->sampled), the bookkeeping and, primed, the next step's embedding.  Otherwise the form's sampler over the logits row lg, with the
// bookkeeping and the next embedding as its fused tail when primed, followed by the advance kernel when not.
int enqueue_tail(mgea_decoder* h, const StepCall& k, float* lg, int n_partials, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    // (with records the EOS id, like the other scalars, is read from them -- the captured graph's form)
    const mgea_decoder::Hist hi = h->hist(k.kind.windowed);
    const StepState s{h->cur_ids, h->ctx_len, h->done, h->row_step, h->n_done, hi.ids, hi.stride, k.pv.eos_id, k.pd};
    const TailArgs t = tail_args(h, s, k.primed ? k.qkv0 : nullptr);
    if (k.kind.form == StepForm::GREEDY) {
        MGEA_REQUIRE(!k.kind.scored && !k.kind.guided && !k.kind.blended && !k.kind.class_penalized, MGEA_EINVAL,
                     "internal: a scored, guided, blended or class-penalised step never takes the greedy form");
        if (k.primed)
            PROF(PC_SAMPLE, launch_argmax_advance_embed(h->pmax_val, h->pmax_idx, n_partials, t, h->sampled, B, st));
        else if (n_partials > 0)
            PROF(PC_SAMPLE, launch_argmax_advance(h->pmax_val, h->pmax_idx, n_partials, s, h->sampled, B, st));
        else
            PROF(PC_ROWOP, launch_advance(h->sampled, s, B, st, nullptr, V));
        return MGEA_OK;
    }
    // guided: every pair's two logits rows become the pair's mixed row, in place, before the sampler reads them
    if (k.kind.guided) PROF(PC_SAMPLE, launch_guidance_mix(lg, B, V, h->guide_partner, h->guide_scale, st));
    // blended: every group's logits rows become the group's mixed row (pairs and groups share no row: either order gives the same rows)
    if (k.kind.blended) PROF(PC_SAMPLE, launch_blend_mix(lg, B, V, h->blend_leader, h->blend_weight, st));
    // class-penalised: behind the mixes (step 0b), every row that is on subtracts its windowed class counts from the row the sampler reads
    if (k.kind.class_penalized)
        PROF(PC_SAMPLE, launch_class_penalty(lg, B, V, h->cpen_class, h->cpen_n_class, hi.ids, hi.stride, h->row_step, h->done, h->cpen_dev, st));
    uint32_t* pres = form_has_presence(k.kind.form) ? h->presence : nullptr;
    SampleCall sc{};
    sc.logits = lg; sc.B = B; sc.V = V;
    sc.params_dev = k.pd; sc.params = k.pv; sc.row_step_dev = h->row_step;
    sc.ids_out = h->sampled; sc.tail = k.primed ? &t : nullptr;
    sc.presence = pres; sc.bias = form_has_bias(k.kind.form) ? h->bias : nullptr;
    if (k.kind.form == StepForm::GRAMMAR)
        sc.grammar = GrammarArgs{h->gram_class, h->gram_next, h->gram_allow, h->gram_state, h->gram_state, h->done,
                                 h->gram_n_state, h->gram_n_class, grammar_words(h->gram_n_class), h->err_flag};
    if (k.kind.truncated) {
        MGEA_REQUIRE(form_has_bias(k.kind.form), MGEA_EINVAL, "internal: a truncated step takes the biased or the grammar form");
        sc.trunc = TruncArgs{h->trunc_dev};
    }
    const int hs = hi.stride;
    if (k.kind.scored)   // fused tail: the sampler files both values at the row's step; otherwise per-step vectors that advance_kernel files
        sc.score = ScoreArgs{hi.forced, hs, k.primed ? hi.lp : h->lp_step, k.primed ? hi.ch : h->ch_step, hs, h->err_flag};
    PROF(PC_SAMPLE, launch_sample(sc, st));
    const ScoreFile sf{h->lp_step, h->ch_step, hi.lp, hi.ch, hs};
    if (!k.primed) PROF(PC_ROWOP, launch_advance(h->sampled, s, B, st, pres, V, k.kind.scored ? &sf : nullptr));
    return MGEA_OK;
}

// The fused step: [embed,] 6 x (qkv, attention, out-proj, fc1, fc2), head (+ per-tile argmax), tail
int enqueue_step_fused(mgea_decoder* h, const StepCall& k, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    if (!k.primed)
        PROF(PC_ROWOP, launch_embed_stats(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, 1, C, V,
                                          c.seq_len, true_positions(c), h->err_flag, st));
    MGEA_REQUIRE(!k.qkv0 || k.primed, MGEA_EINVAL, "internal: the qkv0 table serves primed steps only");
    MGEA_TRY(run_blocks_fused(h, B, 1, nullptr, true, st, false, k.qkv0 != nullptr));
    SkinnyArgs a{};
    a.M = B; a.A = h->x; a.lda = C; a.N = V; a.K = C;
    a.out = k.head_out(h->logits);
    a.ldo = V; a.pmax_val = h->pmax_val; a.pmax_idx = h->pmax_idx;
    DecodeGemmPlan head;   // its partial count is what the greedy tail merges
    PROF(PC_GEMM, decode_gemm(h, 0, 4, a, gemv_ok(h, B, 1, nullptr, true) && gemv_shape_ok(B, V, C), st, &head));
    return enqueue_tail(h, k, a.out, head.n_partials, st);
}

// one decode step on cur_ids: the fused path where the geometry has one, else the slab kernels (never primed: they embed cur_ids)
int enqueue_step(mgea_decoder* h, const StepCall& k, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    if (fused_ok(h, B)) return enqueue_step_fused(h, k, st);
    PROF(PC_ROWOP, launch_embed_ln(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->xn,
                             post ? nullptr : h->lw(0, L_LN1W), post ? nullptr : h->lw(0, L_LN1B), c.ln_eps, B, 1, C,
                             V, c.seq_len, true_positions(c), h->err_flag, st));
    MGEA_TRY(run_blocks(h, B, 1, nullptr, true, true, st));
    int S = 1;
    MGEA_TRY(gemm(h, h->x, C, h->head_w(), B, V, C, &S, st));
    float* lg = k.head_out(h->logits);
    PROF(PC_SAMPLE, launch_logits_argmax(h->slabs, S, slab_floats(B, V), (int)slab_ld(V), h->head_b(), lg, B, V,
                                  k.kind.form == StepForm::GREEDY ? h->sampled : nullptr, st));
    return enqueue_tail(h, k, lg, 0, st);
}

// Which qkv0 table a primed step of B rows reads: 0 the MFMA kernels', 1 the <= 2-row dot-product kernels', -1 none (the layer-0
// in-projection launch stays).  A constant of the handle and B, so every graph of a batch size has one form.
// The 64-row limit is not technical: tests/test_gpu_decoder.py::test_fused_path_beyond_64_rows pins graph_nodes == 32 for a 100-row f32
// step, and existing tests are this project's yardsticks.  64 rows cover the benchmark and the batched server (RequestBatcher).
int qkv0_path(const mgea_decoder* h, int B) {
    if (!h->qkv0_on || h->f16 || h->cfg.pos_mode != MGEA_POS_REFERENCE || !fused_ok(h, B) || B > 64) return -1;
    return gemv_ok(h, B, 1, nullptr, true) ? 1 : 0;
}
const float* qkv0_table(const mgea_decoder* h, int B) {
    const int p = qkv0_path(h, B);
    return p >= 0 && h->qkv0_ready[p] ? h->qkv0_tab[p] : nullptr;
}

// Builds the table of decode path `path` if it is not there: for the ids in chunks of 64 (MFMA) or 2 (GEMV) rows, the embedding at
// position 0 with its statistics, then layer 0's in-projection through decode_gemm -- the step's kernel family and its plan for that
// many rows -- with the chunk's table rows as the output and max_pages = 0, so that the epilogue's page guard keeps it from any KV page.
// The plan of a step is not always the plan of a chunk: pick_mt gives 16-row tiles (MT = 1) to steps of at most 16 rows and to the last,
// short chunk, and 32-row tiles (MT = 2) to the 64-row chunks and to steps of 17..64 rows.  A row's result is the same in both: the
// wave count and the K split do not depend on MT (pick_waves), every 16-row MFMA tile is computed on its own, and the waves' partials are
// added in the same order.  The dot-product kernel likewise computes row 0 of one row and either row of two with the same instruction
// sequence.  tests/test_gpu_qkv0_table.py holds both to the bits (3, 16, 24 and 64 rows; 1 and 2 rows).
// On the call's stream, never inside a capture; x and stats are free between the prefill and the first step.
// Out of device memory: no error, the path keeps its launch (qkv0_no_mem) and mgea_decoder_qkv0_table_bytes says 0.
int ensure_qkv0(mgea_decoder* h, int path, hipStream_t st) {
    if (h->qkv0_ready[path] || h->qkv0_no_mem[path]) return MGEA_OK;
    const auto& c = h->cfg;
    const int C = c.d_model, V = c.vocab;
    if (!h->qkv0_ids) {
        if (h->dev.alloc(&h->qkv0_ids, ((size_t)V + 64) * sizeof(int32_t))) {
            h->qkv0_no_mem[0] = h->qkv0_no_mem[1] = true;
            return MGEA_OK;
        }
        std::vector<int32_t> iota((size_t)V + 64, 0);
        for (int i = 0; i < V; ++i) iota[(size_t)i] = i;
        MGEA_CHECK_HIP(hipMemcpyAsync(h->qkv0_ids, iota.data(), iota.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // iota is a stack-lifetime host buffer (as do_reset's page table)
    }
    if (!h->qkv0_tab[path] && h->dev.alloc(&h->qkv0_tab[path], (size_t)V * 3 * C * sizeof(float))) {
        h->qkv0_no_mem[path] = true;
        return MGEA_OK;
    }
    MGEA_REQUIRE(h->ws_tokens >= 64, MGEA_EINVAL, "internal: qkv0 table build without a 64-row workspace");
    const int rows = path == 1 ? 2 : 64;
    for (int v0 = 0; v0 < V; v0 += rows) {
        const int m = V - v0 < rows ? V - v0 : rows;
        MGEA_TRY(launch_embed_stats(h->qkv0_ids + v0, nullptr, nullptr, h->w(T_TOK), h->w(T_POS), h->x, h->stats, m, 1, C, V, c.seq_len, 0,
                                    nullptr, st));
        SkinnyArgs a{};
        a.M = m; a.eps = c.ln_eps; a.A = h->x; a.lda = C; a.N = 3 * C; a.K = C;
        a.stats_in = h->stats; a.n_part = 2; a.part_cnt = C / 2;
        a.out = h->qkv0_tab[path] + (int64_t)v0 * 3 * C; a.ldo = 3 * C;
        a.pool = h->kv; a.layer = 0; a.page_table = h->page_table; a.max_pages = 0; a.ctx_len = h->qkv0_ids + V;
        a.lens = nullptr; a.T = 1; a.C = C;
        MGEA_TRY(decode_gemm(h, 0, 0, a, path == 1, st));
    }
    h->qkv0_ready[path] = true;
    return MGEA_OK;
}

// The decode step of generate(): the rows' device records; x arrives primed on the fused path.
// windowed: the step opens with the KV window's evict launch, in front of every append of the step (the rule and why it keeps the
// previous tail's layer-0 K | V alive: kv_window.hip); the node does not depend on the step's form.
// guided: the step mixes the pairs' logits rows between the head and the sampler (enqueue_tail); one more node, whatever the pairs are.
// blended: likewise the groups' logits rows, in a launch of its own behind the pairs'; one more node, whatever the groups are.
// class_penalized: the class-penalty launch behind both mixes; one more node, whatever the records are.
// scheduled: behind the evict launch, the launch that applies the rows' prompt schedules (recondition.hip): a row whose segment changes
// gets the new variant's K | V over positions [0, len_b) of its pages before anything of the step reads them; one more node, whatever
// the records say.  (The previous tail's layer-0 K | V of the fed token sits at position ctx_len >= len_b: never in its way.)
int enqueue_gen_step(mgea_decoder* h, int B, const StepKind& kind, hipStream_t st) {
    if (kind.windowed)
        PROF(PC_ROWOP, launch_window_evict(h->page_table, h->max_pages, h->win_S, h->win_R, h->ctx_len, h->done, h->win_evict, B, st));
    if (kind.scheduled) {
        KvPool pool = h->kv;
        if (!tune(TUNE_ATTN_ARITH_PAGES)) pool.arith_batch = 0;   // (as the attention: the switch sends every page id through the table)
        PROF(PC_ROWOP, launch_cond_apply(pool, h->cfg.n_layer, h->page_table, h->max_pages, h->cond_store, h->cond_meta, h->cond_len,
                                         h->cond_sched, h->done, h->row_step, h->gram_state, h->cond_cur_seg, h->cond_switches, B, st));
    }
    return enqueue_step(h, StepCall{B, kind, h->samp_dev, SamplerParams{}, nullptr, fused_ok(h, B), qkv0_table(h, B)}, st);
}

// embedding (+ LN statistics, or through the qkv0 table) of cur_ids into the buffers the next generate() step will read
int prime_gen(mgea_decoder* h, int B, hipStream_t st) {
    if (!fused_ok(h, B)) return MGEA_OK;
    const auto& c = h->cfg;
    if (const float* tab = qkv0_table(h, B))
        return launch_embed_qkv0(h->cur_ids, h->ctx_len, tail_args(h, StepState{}, tab), B, h->err_flag, st);
    return launch_embed_stats(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, 1, c.d_model, c.vocab,
                              c.seq_len, true_positions(c), h->err_flag, st);
}

// The captured graph of `steps` decode steps of `kind` over B rows: from the cache, or captured + instantiated now (least recently used
// entry evicted beyond StepGraphs::CAP, hipres.h).
// steps > 1: that many consecutive decode steps in one graph (switch decoder_graph_steps; the per-step state is in device memory, so the
// steps of a graph are as independent of the host as the graphs are of each other)
int step_graph(mgea_decoder* h, int B, const StepKind& kind, int steps, hipStream_t st, hipGraphExec_t* out) {
    const StepGraphs::Key key{B, steps, kind};
    if (const StepGraphs::Entry* e = h->graphs.find(key)) {
        if (steps == 1) h->n.graph_nodes = e->nodes;
        *out = e->exec;
        return MGEA_OK;
    }
    // the insert below then evicts, and an evicted exec may still be replaying (nothing is launched in between: a capture enqueues no work)
    if (h->graphs.full()) MGEA_CHECK_HIP(hipStreamSynchronize(st));
    MGEA_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = MGEA_OK;
    for (int k = 0; k < steps && rc == MGEA_OK; ++k) rc = enqueue_gen_step(h, B, kind, st);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != MGEA_OK) {
        graph_destroy(g, nullptr);
        return rc;
    }
    MGEA_CHECK_HIP(e);
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) {
        graph_destroy(g, nullptr);
        MGEA_CHECK_HIP(ei);
    }
    size_t nn = 0;
    (void)hipGraphGetNodes(g, nullptr, &nn);
    h->graphs.insert(key, g, ex, (int64_t)nn);
    if (steps == 1) h->n.graph_nodes = (int64_t)nn;
    *out = ex;
    return MGEA_OK;
}

// ---- fp16 engines: prefill of a big batch on the f16 matrix cores --------------------------------------------------------------
// The exact-fp32 kernels run a [64, 1024] prefill at 0.67 of THEIR peak, which is 1/16 of the f16 MFMA rate.  When the cache is empty
// and the batch is big enough for the persistent 256 x 256 GEMM (M / 256 * d_model / 256 >= 256 tiles), an fp16 engine runs the GPT
// block (api_cache.py:51-74, 87-106) on the kernels of the bf16 DistilBERT path with _Float16 operands instead:
//   x (fp16) + (mean, rstd) per row  ->  per layer:
//     qkv  = rstd (x W_in'^T - mean c1) + c2            W_in' = f16(W_in diag(ln1 gamma)): LayerNorm folded into the GEMM (epilogue 3)
//     K | V of the real tokens -> fp16 KV pages;  att = flash attention over qkv (non-causal: the reference has no mask), fp16
//     x'   = att W_out^T + b + x, + row statistics      (epilogue 5, identity tables: the residual is the raw x)
//     hid  = gelu(rstd' (x' W_fc1'^T - mean' c1') + c2')  (epilogue 4)
//     x    = hid W_fc2^T + b + x', + row statistics     (epilogue 5)
//   logits = x W_head^T + b as fp32                      (epilogue 6, N = vocab)
// Everything between two GEMM inputs is fp16 (the residual stream too: 11 significant bits, against bf16's 8 in the DistilBERT mode);
// accumulation, LayerNorm statistics and the softmax are fp32.  W_in' / W_fc1' round gamma * f16(W) once more (the decode path applies
// gamma to the activations instead): the two paths serve models that differ by one fp16 rounding of those two matrices -- inside
// the fp16 mode's tolerance (tests/test_gpu_f16.py compares both with the oracle on the rounded matrices).
bool prefill16_ok(const mgea_decoder* h, int64_t M, bool cache_attn, const float* logits_out) {
    const auto& c = h->cfg;
    if (!h->f16 || cache_attn || c.block_mode != MGEA_BLOCK_PRELN_GELU || !tune(TUNE_DECODER_PREFILL16)) return false;
    if (causal(c)) return false;   // attn16.hip has no causal form: a causal engine's prefills stay on the fp32-activation path
    if (h->dh != 64 || c.d_model % 256 != 0 || c.d_ff % 256 != 0 || c.d_model > 2048) return false;
    if (logits_out && c.vocab % 4 != 0) return false;
    // worth it from the size at which the smallest GEMM (N = d_model) fills the chip with 256 x 256 tiles; switch value 2 (tests)
    // takes every size the kernels accept
    const int64_t tiles = (M / 256) * (c.d_model / 256);
    return M >= 512 && M < (1ll << 24) && tiles >= (tune(TUNE_DECODER_PREFILL16) == 2 ? 8 : 256);
}

int ensure_p16(mgea_decoder* h, int64_t M, hipStream_t st) {
    auto& p = h->p16;
    const auto& c = h->cfg;
    const int64_t C = c.d_model, F = c.d_ff, V = c.vocab, NL = c.n_layer;
    if (M > p.rows) {
        MGEA_CHECK_HIP(hipDeviceSynchronize());
        DevGroup& g = h->dev_p16_rows;   // (alloc() answers MGEA_OK = 0: a chain of || stops at the first failure)
        g.release();
        p.rows = 0;
        const int64_t R = round_up(M, 256);
        if (g.alloc(&p.x0, R * C * 2) || g.alloc(&p.x1, R * C * 2) || g.alloc(&p.qkv, R * 3 * C * 2) || g.alloc(&p.att, R * C * 2) ||
            g.alloc(&p.hid, R * F * 2) || g.alloc(&p.rowstat, R * 2 * 4) || g.alloc(&p.stats_part, R * (C / 256) * 2 * 4) ||
            g.alloc(&p.ident, (R * 2 + 2 * C) * 4) || g.alloc(&p.mask, R * 4)) {
            set_error("decoder: out of device memory for the fp16 prefill workspace (%lld tokens)", (long long)M);
            g.release();
            h->dev_p16_mats.release();
            p = mgea_decoder::Prefill16();   // (the matrices too: a prefill that ran out of memory keeps nothing)
            return MGEA_ENOMEM;
        }
        std::vector<float> idv((size_t)(R * 2 + 2 * C), 0.f);       // (0, 1) per row, then C ones (gamma), then C zeros (beta)
        for (int64_t r = 0; r < R; ++r) idv[(size_t)r * 2 + 1] = 1.f;
        for (int64_t d = 0; d < C; ++d) idv[(size_t)(R * 2 + d)] = 1.f;
        struct Guard { DevGroup* g; ~Guard() { if (g) g->release(); } } unless_filled{&g};   // buffers without their table are no workspace: rows stays 0
        MGEA_CHECK_HIP(hipMemcpy(p.ident, idv.data(), idv.size() * 4, hipMemcpyHostToDevice));
        unless_filled.g = nullptr;
        p.rows = R;
    }
    if (!p.weights_ready) {
        if (!p.w || !p.vec) {
            DevGroup& g = h->dev_p16_mats;
            g.release();
            p.w_off.clear();
            int64_t tot = 0;
            for (int l = 0; l < NL; ++l) {
                p.w_off.push_back(tot); tot += 3 * C * C;
                p.w_off.push_back(tot); tot += C * C;
                p.w_off.push_back(tot); tot += F * C;
                p.w_off.push_back(tot); tot += C * F;
            }
            p.w_off.push_back(tot); tot += round_up(V, 256) * C;     // (rows beyond V are never read: the kernel clamps its row index)
            if (g.alloc(&p.w, tot * 2) || g.alloc(&p.vec, NL * (6 * C + 2 * F) * 4)) {
                g.release();   // both or neither: with p.w set and p.vec null the next prefill would skip this block
                p.w_off.clear();
                set_error("decoder: out of device memory for the fp16 prefill matrices");
                return MGEA_ENOMEM;
            }
        }
        for (int l = 0; l < NL; ++l) {
            MGEA_TRY(launch_fold_ln_weights_bf16(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), (void*)h->p16_w(4 * l + 0),
                                                 h->p16_vec(l, 0), h->p16_vec(l, 1), (int)(3 * C), (int)C, st, 1));
            MGEA_TRY(launch_f32_to_bf16(h->lw(l, L_OUTW), (void*)h->p16_w(4 * l + 1), C * C, st, 1));
            MGEA_TRY(launch_fold_ln_weights_bf16(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), (void*)h->p16_w(4 * l + 2),
                                                 h->p16_vec(l, 2), h->p16_vec(l, 3), (int)F, (int)C, st, 1));
            MGEA_TRY(launch_f32_to_bf16(h->lw(l, L_FC2W), (void*)h->p16_w(4 * l + 3), C * F, st, 1));
        }
        MGEA_TRY(launch_f32_to_bf16(h->head_w(), (void*)h->p16_w(4 * (int)NL), V * C, st, 1));
        p.weights_ready = true;
    }
    return MGEA_OK;
}

int run_prefill16(mgea_decoder* h, const int32_t* ids, const int32_t* lens, int B, int T, float* logits_out, hipStream_t st, bool kv_only_last) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, V = c.vocab, M = B * T, npart = C / 256;
    MGEA_TRY(ensure_p16(h, M, st));
    auto& p = h->p16;
    void *xc = p.x0, *xo = p.x1;
    const float *id_g = p.ident + p.rows * 2, *id_b = id_g + C;
    PROF(PC_ROWOP, launch_dec_embed_f16(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), xc, p.rowstat, lens ? p.mask : nullptr, c.ln_eps, B, T,
                                        C, V, c.seq_len, true_positions(c), h->err_flag, st));
    // K | V of the real tokens reach the fp16 KV pages from inside the attention kernel of their layer (attn16.hip: it has those rows in LDS
    // anyway; round 3 ran a scatter kernel per layer that re-read them from the qkv buffer, on a side stream under the attention).  Only a
    // last block that stops at its K | V (kv_only_last: no attention runs) still uses the scatter kernel.
    for (int l = 0; l < c.n_layer; ++l) {
        const bool last = l + 1 == c.n_layer;
        if (last && kv_only_last) {
            // the logits are dropped (run_blocks): of the last block only K | V -- rows C.. of the stacked projection -- then its scatter
            const BfEpiLn qk{p.rowstat, h->p16_vec(l, 0) + C, nullptr, nullptr, nullptr};
            PROF(PC_GEMM, launch_gemm_bf16(xc, C, (const char*)h->p16_w(4 * l + 0) + (int64_t)C * C * 2, C, h->p16_vec(l, 1) + C, nullptr,
                                           (char*)p.qkv + (int64_t)C * 2, 3 * C, M, 2 * C, C, BEPI_LNFOLD, st, nullptr, &qk, 1));
            PROF(PC_ROWOP, launch_kv_scatter_f16(p.qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
            break;
        }
        const BfEpiLn q{p.rowstat, h->p16_vec(l, 0), nullptr, nullptr, nullptr};
        PROF(PC_GEMM, launch_gemm_bf16(xc, C, h->p16_w(4 * l + 0), C, h->p16_vec(l, 1), nullptr, p.qkv, 3 * C, M, 3 * C, C, BEPI_LNFOLD, st, nullptr, &q, 1));
        const KvPages pages{h->kv, l, h->page_table, h->max_pages};
        if (tune(TUNE_DECODER_PREFILL16_PAGES)) {
            PROF(PC_ATTN_DENSE, launch_attn_bf16(p.qkv, lens ? p.mask : nullptr, p.att, B, T, c.n_head, h->dh, st, 1, &pages));
        } else {
            PROF(PC_ROWOP, launch_kv_scatter_f16(p.qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
            PROF(PC_ATTN_DENSE, launch_attn_bf16(p.qkv, lens ? p.mask : nullptr, p.att, B, T, c.n_head, h->dh, st, 1));
        }
        const BfEpiLn o{p.ident, nullptr, id_g, id_b, p.stats_part};
        PROF(PC_GEMM, launch_gemm_bf16(p.att, C, h->p16_w(4 * l + 1), C, h->lw(l, L_OUTB), xc, xo, C, M, C, C, BEPI_RES_LN, st, nullptr, &o, 1));
        PROF(PC_ROWOP, launch_ln_rowstat(p.stats_part, p.rowstat, M, npart, C, c.ln_eps, st));
        const BfEpiLn f1{p.rowstat, h->p16_vec(l, 2), nullptr, nullptr, nullptr};
        PROF(PC_GEMM, launch_gemm_bf16(xo, C, h->p16_w(4 * l + 2), C, h->p16_vec(l, 3), nullptr, p.hid, F, M, F, C, BEPI_LNFOLD_GELU, st, nullptr, &f1, 1));
        const BfEpiLn f2{p.ident, nullptr, id_g, id_b, last ? nullptr : p.stats_part};
        // reads FC1's big output: walk the tiles backwards (reverse = 1; gemm16.hip)
        PROF(PC_GEMM, launch_gemm_bf16(p.hid, F, h->p16_w(4 * l + 3), F, h->lw(l, L_FC2B), xo, xc, C, M, C, F, BEPI_RES_LN, st, nullptr, &f2, 1, 1));
        if (!last) PROF(PC_ROWOP, launch_ln_rowstat(p.stats_part, p.rowstat, M, npart, C, c.ln_eps, st));
    }
    if (logits_out)
        PROF(PC_GEMM, launch_gemm_bf16(xc, C, h->p16_w(4 * c.n_layer), C, h->head_b(), nullptr, logits_out, V, M, V, C, BEPI_BIAS_F32, st, nullptr, nullptr, 1));
    h->n.prefill16_forwards += 1;
    return MGEA_OK;
}

int do_reset(mgea_decoder* h, int B, int max_len, hipStream_t st) {
    const auto& c = h->cfg;
    MGEA_REQUIRE(B > 0 && B <= c.max_batch, MGEA_ECAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
    MGEA_REQUIRE(max_len > 0 && max_len <= c.max_ctx, MGEA_ECAPACITY, "context %d exceeds max_ctx %d", max_len, c.max_ctx);
    const int ppr = ceil_div(max_len, MGEA_KV_PAGE_TOKENS);
    MGEA_REQUIRE((int64_t)B * ppr <= h->kv.n_pages, MGEA_ECAPACITY, "KV pool too small: need %d pages", B * ppr);
    // page allocation: logical page j of row b -> physical j*B + b (the rows' j-th pages are
    // neighbours, so a decode step streams one contiguous region per page index)
    std::vector<int32_t> pt((size_t)c.max_batch * h->max_pages, 0);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < ppr; ++j) pt[(size_t)b * h->max_pages + j] = j * B + b;
    h->kv.arith_batch = B;   // the rule above, for kernels that would rather compute a page id than load it (attn_paged.hip)
    MGEA_CHECK_HIP(hipMemcpyAsync(h->page_table, pt.data(), pt.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));  // pt is a stack-lifetime host buffer
    const size_t nb = (size_t)c.max_batch * sizeof(int32_t);
    MGEA_CHECK_HIP(hipMemsetAsync(h->ctx_len, 0, nb, st));
    MGEA_CHECK_HIP(hipMemsetAsync(h->cur_ids, 0, nb, st));
    MGEA_CHECK_HIP(hipMemsetAsync(h->done, 0, nb, st));
    MGEA_CHECK_HIP(hipMemsetAsync(h->row_step, 0, nb, st));
    MGEA_CHECK_HIP(hipMemsetAsync(h->n_done, 0, 16, st));
    h->cur_batch = B;
    h->reserved_len = ppr * MGEA_KV_PAGE_TOKENS < c.max_ctx ? ppr * MGEA_KV_PAGE_TOKENS : c.max_ctx;
    h->host_max_len = 0;
    h->host_min_len = 0;
    h->win_dirty = false;
    return MGEA_OK;
}

int do_forward(mgea_decoder* h, const int32_t* ids, const int32_t* lens, int B, int T, float* logits_out,
               hipStream_t st) {
    const auto& c = h->cfg;
    MGEA_REQUIRE(ids, MGEA_EINVAL, "forward: ids is NULL");
    MGEA_REQUIRE(h->cur_batch > 0, MGEA_EINVAL, "forward: call mgea_decoder_reset first");
    MGEA_REQUIRE(B == h->cur_batch, MGEA_EINVAL, "forward: batch %d differs from the reset batch %d", B, h->cur_batch);
    MGEA_REQUIRE(!h->win_dirty, MGEA_EINVAL, "forward: the cache holds a windowed generation; call mgea_decoder_reset first");
    MGEA_REQUIRE(T > 0, MGEA_EINVAL, "forward: T must be positive");
    // the reference fails with a broadcast RuntimeError when T exceeds the position table (api_cache.py:99)
    MGEA_REQUIRE(T <= c.seq_len, MGEA_EINVAL, "T=%d exceeds the position table (%d rows)", T, c.seq_len);
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    if (!post)
        MGEA_REQUIRE(h->host_max_len + T <= h->reserved_len, MGEA_ECAPACITY,
                     "context %d + %d new tokens exceeds the reserved %d", h->host_max_len, T, h->reserved_len);
    const int C = c.d_model, V = c.vocab;
    const int64_t M = (int64_t)B * T;
    MGEA_REQUIRE(M < (1ll << 30), MGEA_EINVAL, "forward: too many tokens");
    MGEA_TRY(ensure_ws(h, M));
    const bool cache_attn = (!post) && h->host_max_len > 0;
    const bool p16 = !fused_ok(h, (int)M) && prefill16_ok(h, M, cache_attn, logits_out);
    const bool kv_only_last = !logits_out && !post && !tune(TUNE_DECODER_PREFILL_FULL);   // logits dropped: the last block stops at its K | V
    if (p16) {
        MGEA_TRY(run_prefill16(h, ids, lens, B, T, logits_out, st, kv_only_last));   // computes the logits itself (fp32 output of its head GEMM)
    } else if (fused_ok(h, (int)M)) {
        MGEA_TRY(launch_embed_stats(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, T, C, V,
                                    c.seq_len, true_positions(c), h->err_flag, st));
        MGEA_TRY(run_blocks_fused(h, B, T, lens, cache_attn, st, kv_only_last));
    } else {
        MGEA_TRY(launch_embed_ln(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->xn,
                                 post ? nullptr : h->lw(0, L_LN1W), post ? nullptr : h->lw(0, L_LN1B), c.ln_eps, B, T, C,
                                 V, c.seq_len, (!post) && true_positions(c), h->err_flag, st));
        MGEA_TRY(run_blocks(h, B, T, lens, cache_attn, !post, st, kv_only_last));
    }
    if (p16) {
    } else if (logits_out && fused_ok(h, (int)M)) {
        SkinnyArgs a{};  // x is k-tiled on the fused path: the head is a decode GEMM (LOGITS epilogue) on the tiled weights
        a.M = (int)M; a.A = h->x; a.lda = C; a.N = V; a.K = C;
        a.out = logits_out; a.ldo = V;
        MGEA_TRY(decode_gemm(h, 0, 4, a, false, st));
    } else if (logits_out) {
        for (int64_t r0 = 0; r0 < M; r0 += 4096) {
            const int rows = (int)((M - r0) < 4096 ? (M - r0) : 4096);
            if (V % 4 == 0 && gemm_direct_epilogue_ok(rows, V)) {   // bias inside the GEMM: no slab write + read of rows x V floats.  (Same sums as the slab form wherever that
                                                                    // would not split K: from 256 tiles on.  A remainder chunk of 128..255 tiles used to run with K split; its
                                                                    // logits differ from that form in the last bits of the fp32 sums, within the 5e-6 the long-prompt test observes.)
                PROF(PC_GEMM, launch_gemm_f32_bias_act(h->x + r0 * C, C, h->head_w(), C, h->head_b(), logits_out + r0 * V, V, rows, V, C, ACT_NONE, st));
                continue;
            }
            int S = 1;
            MGEA_TRY(gemm(h, h->x + r0 * C, C, h->head_w(), rows, V, C, &S, st));
            MGEA_TRY(launch_bias_act(h->slabs, S, slab_floats(rows, V), (int)slab_ld(V), h->head_b(),
                                     logits_out + r0 * V, V, rows, V, ACT_NONE, st));
        }
    }
    if (!post) {
        MGEA_TRY(launch_add_lens(h->ctx_len, lens, T, B, st));
        h->host_max_len += T;
    }
    MGEA_TRY(launch_take_last(ids, lens, h->cur_ids, B, T, st));
    return MGEA_OK;
}

}  // namespace

extern "C" {

int mgea_decoder_arena_layout(const mgea_decoder_config* cfg, int64_t* offsets_floats, int32_t* n_tensors,
                              int64_t* total_floats) {
    MGEA_TRY(validate(cfg));
    std::vector<int64_t> offs;
    int64_t total = 0;
    const int n = arena_layout(*cfg, &offs, &total);
    if (offsets_floats)
        for (int i = 0; i < n; ++i) offsets_floats[i] = offs[i];
    if (n_tensors) *n_tensors = n;
    if (total_floats) *total_floats = total;
    return MGEA_OK;
}

// (Re)derive the fragment-ordered matrices of the fused decode path from the arena; synchronous.
static int build_tiled_weights(mgea_decoder* h, hipStream_t st) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, V = c.vocab;
    if (!h->wt) {
        int64_t total = 0;
        h->wt_off.clear();
        for (int l = 0; l < c.n_layer; ++l) {
            h->wt_off.push_back(total); total += wtile_floats(3 * C, C);
            h->wt_off.push_back(total); total += wtile_floats(C, C);
            h->wt_off.push_back(total); total += wtile_floats(F, C);
            h->wt_off.push_back(total); total += wtile_floats(C, F);
        }
        h->wt_off.push_back(total); total += wtile_floats(V, C);
        if (h->dev.alloc(&h->wt, (size_t)total * (h->f16 ? 2 : 4)) || h->dev.alloc(&h->lnv, (size_t)c.n_layer * (6 * C + 2 * F) * sizeof(float))) {
            set_error("decoder_create: allocation of the decode-layout weights (%lld MB) failed", (long long)(total * (h->f16 ? 2 : 4) >> 20));
            return MGEA_ENOMEM;   // (wt may stay without lnv: create destroys the handle, and the check below stops anyone else)
        }
    }
    MGEA_REQUIRE(h->lnv, MGEA_EINVAL, "internal: decode-layout weights half built");
    if (h->f16) {
        // private model copy: the caller's arena with the five matrix kinds rounded to fp16 (fp32 storage) ...
        float* own = h->arena_own;
        MGEA_CHECK_HIP(hipMemcpyAsync(own, h->arena_src, (size_t)h->arena_total * sizeof(float), hipMemcpyDeviceToDevice, st));
        const int mats[4] = {L_INW, L_OUTW, L_FC1W, L_FC2W};
        const int64_t msz[4] = {3ll * C * C, (int64_t)C * C, (int64_t)F * C, (int64_t)C * F};
        for (int l = 0; l < c.n_layer; ++l)
            for (int j = 0; j < 4; ++j) MGEA_TRY(launch_round_f16_inplace(own + h->off[2 + l * L_COUNT + mats[j]], msz[j], st));
        MGEA_TRY(launch_round_f16_inplace(own + h->off[2 + c.n_layer * L_COUNT], (int64_t)V * C, st));
        // ... and its fp16 fragments for the decode path; LayerNorm's gamma is applied on the activation side (gemm_skinny.hip)
        _Float16* wt = static_cast<_Float16*>(h->wt);
        for (int l = 0; l < c.n_layer; ++l) {
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_INW), 3 * C, C, wt + h->wt_off[4 * l + 0], st));
            MGEA_TRY(launch_ln_vectors(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), 3 * C, C,
                                       const_cast<float*>(h->qkv_c1(l)), const_cast<float*>(h->qkv_c2(l)), st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_OUTW), C, C, wt + h->wt_off[4 * l + 1], st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_FC1W), F, C, wt + h->wt_off[4 * l + 2], st));
            MGEA_TRY(launch_ln_vectors(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), F, C,
                                       const_cast<float*>(h->fc1_c1(l)), const_cast<float*>(h->fc1_c2(l)), st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_FC2W), C, F, wt + h->wt_off[4 * l + 3], st));
        }
        MGEA_TRY(launch_tile_weights_f16(h->head_w(), V, C, wt + h->wt_off[4 * c.n_layer], st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
        return MGEA_OK;
    }
    float* wt = static_cast<float*>(h->wt);
    for (int l = 0; l < c.n_layer; ++l) {
        MGEA_TRY(launch_ln_fold(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), 3 * C, C,
                                wt + h->wt_off[4 * l + 0], const_cast<float*>(h->qkv_c1(l)), const_cast<float*>(h->qkv_c2(l)), st));
        MGEA_TRY(launch_tile_weights(h->lw(l, L_OUTW), C, C, wt + h->wt_off[4 * l + 1], st));
        MGEA_TRY(launch_ln_fold(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), F, C,
                                wt + h->wt_off[4 * l + 2], const_cast<float*>(h->fc1_c1(l)), const_cast<float*>(h->fc1_c2(l)), st));
        MGEA_TRY(launch_tile_weights(h->lw(l, L_FC2W), C, F, wt + h->wt_off[4 * l + 3], st));
    }
    MGEA_TRY(launch_tile_weights(h->head_w(), V, C, wt + h->wt_off[4 * c.n_layer], st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    return MGEA_OK;
}

int mgea_decoder_create(const mgea_decoder_config* cfg, const float* arena_dev, mgea_decoder** out) {
    MGEA_TRY(validate(cfg));
    MGEA_REQUIRE(arena_dev && out, MGEA_EINVAL, "decoder_create: NULL argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: the MI355X path has no CPU fallback");
        return MGEA_ENODEVICE;
    }
    { DeviceInfo di; MGEA_TRY(device_info(&di)); }   // cached now: launchers ask for it inside graph capture
    mgea_decoder* h = new mgea_decoder();   // from here on every failure goes through destroy
    h->cfg = *cfg;
    h->arena = h->arena_src = arena_dev;
    h->f16 = cfg->dtype == MGEA_DTYPE_F16;
    int64_t total = 0;
    arena_layout(*cfg, &h->off, &total);
    h->arena_total = total;
    h->dh = cfg->d_model / cfg->n_head;
    h->force_unfused = tune(TUNE_DECODER_UNFUSED) == 1;   // A/B switches (tools/README.md), latched per engine
    h->no_gemv = tune(TUNE_DECODER_NOGEMV) == 1;
    h->no_graph = tune(TUNE_DECODER_NOGRAPH) == 1;
    h->qkv0_on = tune(TUNE_DECODER_QKV0_TABLE) == 1;
    h->pages_per_row_cap = ceil_div(cfg->max_ctx, MGEA_KV_PAGE_TOKENS);
    h->max_pages = h->pages_per_row_cap;
    h->kv.n_pages = cfg->max_batch * h->pages_per_row_cap;
    h->kv.H = cfg->n_head;
    h->kv.dh = h->dh;
    h->kv.f16 = h->f16 ? 1 : 0;
    h->kv.layer_stride = (int64_t)h->kv.n_pages * 2 * cfg->n_head * h->kv.page_elems();
    const size_t pool_bytes = (size_t)h->kv.layer_stride * cfg->n_layer * h->kv.elt_bytes();
    auto fail = [&](int code, const char* what) {
        set_error("decoder_create: %s", what);
        mgea_decoder_destroy(h);
        return code;
    };
    DevGroup& g = h->dev;   // (alloc() answers MGEA_OK = 0: a chain of || stops at the first failure)
    if (h->f16) {
        if (g.alloc(&h->arena_own, (size_t)total * sizeof(float)))
            return fail(MGEA_ENOMEM, "allocation of the fp16-rounded model copy failed");
        h->arena = h->arena_own;   // filled by build_tiled_weights below
    }
    if (cfg->block_mode == MGEA_BLOCK_PRELN_GELU) {
        if (g.alloc(&h->kv.base, pool_bytes)) return fail(MGEA_ENOMEM, "KV pool allocation failed");
        if (hipMemset(h->kv.base, 0, pool_bytes) != hipSuccess) return fail(MGEA_EHIP, "KV pool memset failed");
    }
    const size_t nb = (size_t)cfg->max_batch * sizeof(int32_t);
    h->ids_hist_stride = cfg->max_ctx;
    if (g.alloc(&h->page_table, nb * h->max_pages) || g.alloc(&h->ctx_len, nb) || g.alloc(&h->cur_ids, nb) || g.alloc(&h->done, nb) ||
        g.alloc(&h->row_step, nb) || g.alloc(&h->sampled, nb) || g.alloc(&h->n_done, 16) ||
        g.alloc(&h->samp_dev, cfg->max_batch * sizeof(SamplerParams)) ||
        h->pinned.alloc(&h->samp_stage, cfg->max_batch * sizeof(SamplerParams)) ||
        hipEventCreateWithFlags(&h->stage_free.ev, hipEventDisableTiming) != hipSuccess ||
        g.alloc(&h->err_flag, 16) || g.alloc(&h->presence, (size_t)cfg->max_batch * presence_words(cfg->vocab) * sizeof(uint32_t)) ||
        g.alloc(&h->ids_hist, nb * h->ids_hist_stride))
        return fail(MGEA_ENOMEM, "state allocation failed");
    h->attn_split.max_split = MGEA_ATTN_MAX_SPLIT;
    h->attn_split.max_items = MGEA_ATTN_SPLIT_ITEMS;   // attn_split_count(): (row, head) pairs, one query each
    const size_t nhist = (size_t)cfg->max_batch * h->ids_hist_stride;
    if (g.alloc(&h->attn_split.part, (size_t)MGEA_ATTN_SPLIT_ITEMS * MGEA_ATTN_MAX_SPLIT * attn_part_floats(h->dh) * sizeof(float)) ||
        g.alloc(&h->attn_split.count, MGEA_ATTN_SPLIT_ITEMS * sizeof(int32_t)) ||
        // (the logit bias came after the state buffers above, which keep the places they had before it existed: DESIGN.md §5)
        g.alloc(&h->bias, (size_t)cfg->max_batch * cfg->vocab * sizeof(float)) || g.alloc(&h->forced, nhist * sizeof(int32_t)) ||
        g.alloc(&h->lp_hist, nhist * sizeof(float)) || g.alloc(&h->ch_hist, nhist * sizeof(float)) ||
        g.alloc(&h->lp_step, cfg->max_batch * sizeof(float)) || g.alloc(&h->ch_step, cfg->max_batch * sizeof(float)) ||
        // (the grammar's buffers came after those, for the same reason)
        g.alloc(&h->gram_state, nb) || g.alloc(&h->gram_class, (size_t)cfg->vocab * sizeof(int32_t)) ||
        g.alloc(&h->gram_next, (size_t)MGEA_GRAMMAR_MAX_CELLS * sizeof(int32_t)) ||
        g.alloc(&h->gram_allow, ((size_t)MGEA_GRAMMAR_MAX_CELLS / 32 + MGEA_GRAMMAR_MAX_STATES) * sizeof(uint32_t)) ||
        h->pinned.alloc(&h->gram_stage, nb) ||
        // (and the guidance pairs after the grammar's)
        g.alloc(&h->guide_partner, nb) || g.alloc(&h->guide_scale, cfg->max_batch * sizeof(float)) ||
        h->pinned.alloc(&h->guide_stage, 2 * nb) ||
        // (and the truncation records after the guidance pairs)
        g.alloc(&h->trunc_dev, cfg->max_batch * sizeof(mgea_row_truncation)) ||
        h->pinned.alloc(&h->trunc_stage, cfg->max_batch * sizeof(mgea_row_truncation)) ||
        // (and the blend groups after the truncation records)
        g.alloc(&h->blend_leader, nb) || g.alloc(&h->blend_weight, cfg->max_batch * sizeof(float)) ||
        h->pinned.alloc(&h->blend_stage, 2 * nb))
        return fail(MGEA_ENOMEM, "state allocation failed");
    if (hipMemset(h->forced, 0xff, nhist * sizeof(int32_t)) != hipSuccess ||
        hipMemset(h->guide_partner, 0xff, nb) != hipSuccess || hipMemset(h->guide_scale, 0, cfg->max_batch * sizeof(float)) != hipSuccess ||
        hipMemset(h->attn_split.count, 0, MGEA_ATTN_SPLIT_ITEMS * sizeof(int32_t)) != hipSuccess ||
        hipMemset(h->gram_state, 0xff, nb) != hipSuccess ||
        hipMemset(h->trunc_dev, 0, cfg->max_batch * sizeof(mgea_row_truncation)) != hipSuccess ||
        hipMemset(h->blend_leader, 0xff, nb) != hipSuccess || hipMemset(h->blend_weight, 0, cfg->max_batch * sizeof(float)) != hipSuccess ||
        hipMemset(h->page_table, 0, nb * h->max_pages) != hipSuccess || hipMemset(h->ctx_len, 0, nb) != hipSuccess ||
        hipMemset(h->done, 0, nb) != hipSuccess || hipMemset(h->row_step, 0, nb) != hipSuccess ||
        hipMemset(h->cur_ids, 0, nb) != hipSuccess || hipMemset(h->n_done, 0, 16) != hipSuccess ||
        hipMemset(h->samp_dev, 0, cfg->max_batch * sizeof(SamplerParams)) != hipSuccess || hipMemset(h->err_flag, 0, 16) != hipSuccess)
        return fail(MGEA_EHIP, "state memset failed");
    int rc = ensure_ws(h, cfg->max_batch > 64 ? cfg->max_batch : 64);
    if (rc == MGEA_OK && fused_geometry(*cfg)) rc = build_tiled_weights(h, nullptr);
    // (causal engines only, and last in the group: every other engine allocates what it always did, in the same order)
    if (rc == MGEA_OK && causal(*cfg) && g.alloc(&h->lens_m1, nb)) {
        set_error("decoder_create: state allocation failed");
        rc = MGEA_ENOMEM;
    }
    if (rc != MGEA_OK) {
        mgea_decoder_destroy(h);
        return rc;
    }
    *out = h;
    return MGEA_OK;
}

int mgea_decoder_refresh_weights(mgea_decoder* h, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    h->p16.weights_ready = false;   // rebuilt from the refreshed model copy at the next big-batch prefill
    h->qkv0_ready[0] = h->qkv0_ready[1] = false;   // and the qkv0 tables at the next generation, in place (the graphs keep their pointers)
    if (!fused_geometry(h->cfg)) return MGEA_OK;
    return build_tiled_weights(h, (hipStream_t)stream);
}

int mgea_decoder_destroy(mgea_decoder* h) {
    if (!h) return MGEA_OK;
    (void)hipDeviceSynchronize();
    delete h;   // every resource goes with its owner (devmem.h, hipres.h)
    return MGEA_OK;
}

int mgea_decoder_reset(mgea_decoder* h, int32_t batch, int32_t max_len, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    return do_reset(h, batch, max_len, (hipStream_t)stream);
}

int mgea_decoder_forward(mgea_decoder* h, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t T,
                         float* logits_out_dev, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    return do_forward(h, ids_dev, lens_dev, B, T, logits_out_dev, (hipStream_t)stream);
}

int mgea_decoder_step(mgea_decoder* h, const int32_t* ids_in_dev, const mgea_sampler_config* s, int32_t* ids_out_dev,
                      float* logits_out_dev, void* stream) {
    MGEA_REQUIRE(h && s, MGEA_EINVAL, "decoder_step: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    MGEA_REQUIRE(h->cfg.block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "decoder_step needs the KV-cache block mode");
    MGEA_REQUIRE(h->cur_batch > 0, MGEA_EINVAL, "decoder_step: call reset/forward first");
    MGEA_REQUIRE(!h->win_dirty, MGEA_EINVAL, "decoder_step: the cache holds a windowed generation; call mgea_decoder_reset first");
    MGEA_REQUIRE(h->host_max_len + 1 <= h->reserved_len, MGEA_ECAPACITY, "context %d + 1 exceeds the reserved %d",
                 h->host_max_len, h->reserved_len);
    const int B = h->cur_batch;
    if (ids_in_dev)
        MGEA_CHECK_HIP(hipMemcpyAsync(h->cur_ids, ids_in_dev, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    // eager single step: the scalars travel by value
    MGEA_TRY(enqueue_step(h, StepCall{B, StepKind{step_form(s->top_k == 1, false, false)}, nullptr, sampler_params(*s), logits_out_dev, false}, st));
    h->host_max_len += 1;
    if (ids_out_dev)
        MGEA_CHECK_HIP(hipMemcpyAsync(ids_out_dev, h->sampled, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return MGEA_OK;
}

}  // extern "C"

namespace {
// The buffers of a scheduled generation (dev_cond), big enough for `bytes` of store.  They are allocated, and regrown, by scheduled
// calls only; a regrow frees pointers the scheduled graphs hold, so it synchronises and drops those.
int ensure_cond(mgea_decoder* h, int64_t bytes, hipStream_t st) {
    if (h->cond_store && bytes <= h->cond_bytes) return MGEA_OK;
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying, a freed store still be read
    h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.scheduled; });
    DevGroup& g = h->dev_cond;
    g.release();
    h->cond_bytes = 0;
    const size_t mb = (size_t)h->cfg.max_batch;
    if ((!h->cond_stage && h->pinned.alloc(&h->cond_stage, mb * sizeof(mgea_row_schedule))) || g.alloc(&h->cond_store, (size_t)bytes) ||
        g.alloc(&h->cond_sched, mb * sizeof(mgea_row_schedule)) || g.alloc(&h->cond_cur_seg, mb * sizeof(int32_t)) ||
        g.alloc(&h->cond_switches, 16) || g.alloc(&h->cond_meta, 16) || g.alloc(&h->cond_len, mb * sizeof(int32_t))) {
        g.release();
        set_error("decoder_generate_rows_scheduled: allocation of the conditioning store (%lld MB) failed", (long long)(bytes >> 20));
        return MGEA_ENOMEM;
    }
    h->cond_bytes = bytes;
    return MGEA_OK;
}

// ---- generate(): plan, prefill, stage, run, finish ------------------------------------------------------------------------------
// do_generate runs a GenRequest (gen_plan.h) in five phases, each a function of the request and its plan; the caller holds h->mu.
GenLimits gen_limits(const mgea_decoder* h) {
    const auto& c = h->cfg;
    return GenLimits{c.vocab, c.max_batch, c.max_ctx, c.block_mode, h->win_S, h->win_R, h->win_max_steps, h->gram_n_state, h->cpen_n_class};
}

// A guidance shadow row runs on its conditional row's inputs -- same inputs, same id --, a non-leader member of a blend group on its
// leader's, and this is the one place that hands them over.
// `part` names what the caller has just filled for the callers' rows:
//   PRESENCE  the seeded bitmaps: a pair's set is the conditional prompt plus the generated ids, and both tails add the same ids
//   RECORDS   the pinned staging arrays: the sampler record -- seed, Philox stream, budget and all --, the grammar start state, the
//             truncation record and the class-penalty record (the rows are fed the same ids: the same counts, the same function)
//   BIAS      the engine's bias rows: the shadow adds its conditional row's vector (its record says bias_on as that one's does)
//   FORCED    the engine's forced-id rows: the shadow is told the ids its conditional row is told
enum class Mirror { PRESENCE, RECORDS, BIAS, FORCED };
int mirror_shadow_rows(mgea_decoder* h, const GenRequest& q, const GenPlan& p, Mirror part, hipStream_t st) {
    if (!p.kind.guided && !p.kind.blended) return MGEA_OK;
    const size_t V = (size_t)h->cfg.vocab, pw = (size_t)presence_words(h->cfg.vocab);
    const mgea_decoder::Hist hi = h->hist(p.kind.windowed);
    const size_t hs = (size_t)hi.stride;
    // row u takes what row b has: u = b's shadow row, or u = a member of the group b leads (a row is never both: plan_generation)
    for (int u = 0; u < q.B; ++u) {
        int b = -1;
        if (p.kind.blended && q.blend[u].leader >= 0 && q.blend[u].leader != u) b = q.blend[u].leader;
        for (int c = 0; p.kind.guided && b < 0 && c < q.B; ++c)
            if (q.guide[c].shadow_row == u) b = c;
        if (b < 0) continue;
        switch (part) {
        case Mirror::PRESENCE:
            MGEA_CHECK_HIP(hipMemcpyAsync(h->presence + (size_t)u * pw, h->presence + (size_t)b * pw, pw * sizeof(uint32_t),
                                          hipMemcpyDeviceToDevice, st));
            break;
        case Mirror::RECORDS:
            h->samp_stage[u] = h->samp_stage[b];
            if (p.grammar) h->gram_stage[u] = q.start_states[b];
            if (p.truncated) h->trunc_stage[u] = h->trunc_stage[b];
            if (p.kind.class_penalized) h->cpen_stage[u] = h->cpen_stage[b];
            break;
        case Mirror::BIAS:
            if (h->samp_stage[b].bias_on)
                MGEA_CHECK_HIP(hipMemcpyAsync(h->bias + (size_t)u * V, h->bias + (size_t)b * V, V * sizeof(float), hipMemcpyDeviceToDevice, st));
            break;
        case Mirror::FORCED:
            MGEA_CHECK_HIP(hipMemcpyAsync(hi.forced + (size_t)u * hs, hi.forced + (size_t)b * hs, (size_t)q.n_steps * sizeof(int32_t),
                                          hipMemcpyDeviceToDevice, st));
            break;
        }
    }
    return MGEA_OK;
}

// Prefill: for a scheduled call the variants' prefills and gathers, then the generation's own reset and prefill (logits dropped,
// api_cache.py:163) and the presence seed.  Leaves the cache, cur_ids and the host mirror as the first step reads them.
int gen_prefill(mgea_decoder* h, const GenRequest& q, const GenPlan& p, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = q.B, Tp = q.Tp;
    const bool windowed = p.kind.windowed;
    // positions [0, lens) of the prefill that has just finished -> segment sg of the conditioning store (the pool as the attention sees
    // it: the allocation rule where the prefill's pages follow it, the table otherwise)
    auto gather = [&](int sg) {
        KvPool pool = h->kv;
        if (!tune(TUNE_ATTN_ARITH_PAGES)) pool.arith_batch = 0;
        return launch_cond_gather(pool, c.n_layer, h->page_table, h->max_pages, q.lens, Tp, h->cond_store, sg, q.n_seg_max, Tp, h->cond_meta,
                                  h->cond_len, B, st);
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
        MGEA_CHECK_HIP(hipMemsetAsync(h->win_evict, 0, (size_t)c.max_batch * sizeof(int32_t), st));
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
        MGEA_CHECK_HIP(hipMemsetAsync(h->cond_cur_seg, 0, (size_t)c.max_batch * sizeof(int32_t), st));
        MGEA_CHECK_HIP(hipMemsetAsync(h->cond_switches, 0, 16, st));
    }
    h->win_dirty = windowed;
    if (form_has_presence(p.kind.form)) {   // every row's set starts as its real prompt tokens
        MGEA_TRY(launch_presence_seed(q.prompt_ids, q.lens, B, Tp, c.vocab, h->presence, st));
        MGEA_TRY(mirror_shadow_rows(h, q, p, Mirror::PRESENCE, st));
    }
    return MGEA_OK;
}

// Stage: everything the steps read besides the cache goes into engine memory, stream-ordered and without a host sync -- the rows'
// records, bias vectors, grammar states, pairs, schedules and forced ids.  The captured graphs point at the engine's buffers, so one
// graph serves every step of every request.
int gen_stage(mgea_decoder* h, const GenRequest& q, const GenPlan& p, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = q.B;
    if (q.rows) {
        // the pinned staging arrays are free once the previous call's copies out of them have run
        MGEA_CHECK_HIP(hipEventSynchronize(h->stage_free.ev));
        build_row_records(q.rows, q.lrows, B, q.n_steps, h->samp_stage);
        for (int b = 0; p.grammar && b < B; ++b) h->gram_stage[b] = q.start_states[b];
        for (int b = 0; p.truncated && b < B; ++b) h->trunc_stage[b] = q.trunc[b];
        for (int b = 0; p.kind.class_penalized && b < B; ++b) h->cpen_stage[b] = q.cpen[b];
        MGEA_TRY(mirror_shadow_rows(h, q, p, Mirror::RECORDS, st));
        for (int b = 0; p.biased && b < B; ++b)
            if (q.lrows[b].bias_dev)   // the row's vector -> its row of the engine's buffer, which the graphs point at
                MGEA_CHECK_HIP(hipMemcpyAsync(h->bias + (size_t)b * c.vocab, q.lrows[b].bias_dev, (size_t)c.vocab * sizeof(float),
                                              hipMemcpyDeviceToDevice, st));
        if (p.biased) MGEA_TRY(mirror_shadow_rows(h, q, p, Mirror::BIAS, st));
        MGEA_CHECK_HIP(hipMemcpyAsync(h->samp_dev, h->samp_stage, (size_t)B * sizeof(SamplerParams), hipMemcpyHostToDevice, st));
        if (p.grammar)
            MGEA_CHECK_HIP(hipMemcpyAsync(h->gram_state, h->gram_stage, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (p.truncated)
            MGEA_CHECK_HIP(hipMemcpyAsync(h->trunc_dev, h->trunc_stage, (size_t)B * sizeof(mgea_row_truncation), hipMemcpyHostToDevice, st));
        if (p.kind.class_penalized)
            MGEA_CHECK_HIP(hipMemcpyAsync(h->cpen_dev, h->cpen_stage, (size_t)B * sizeof(mgea_row_class_penalty), hipMemcpyHostToDevice, st));
        if (p.kind.guided) {   // the pairs and their scales: the guided graphs read the engine's two vectors
            float* scale_stage = reinterpret_cast<float*>(h->guide_stage + c.max_batch);
            for (int b = 0; b < B; ++b) {
                h->guide_stage[b] = q.guide[b].shadow_row;
                scale_stage[b] = q.guide[b].shadow_row >= 0 ? q.guide[b].scale : 0.f;
            }
            MGEA_CHECK_HIP(hipMemcpyAsync(h->guide_partner, h->guide_stage, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
            MGEA_CHECK_HIP(hipMemcpyAsync(h->guide_scale, scale_stage, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
        }
        if (p.kind.blended) {   // the groups and their weights: the blended graphs read the engine's two vectors
            float* weight_stage = reinterpret_cast<float*>(h->blend_stage + c.max_batch);
            for (int b = 0; b < B; ++b) {
                h->blend_stage[b] = q.blend[b].leader;
                weight_stage[b] = q.blend[b].leader >= 0 ? q.blend[b].weight : 0.f;
            }
            MGEA_CHECK_HIP(hipMemcpyAsync(h->blend_leader, h->blend_stage, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
            MGEA_CHECK_HIP(hipMemcpyAsync(h->blend_weight, weight_stage, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
        }
        if (p.kind.scheduled) {
            for (int b = 0; b < B; ++b) h->cond_stage[b] = q.sched[b];
            MGEA_CHECK_HIP(hipMemcpyAsync(h->cond_sched, h->cond_stage, (size_t)B * sizeof(mgea_row_schedule), hipMemcpyHostToDevice, st));
        }
        MGEA_CHECK_HIP(hipEventRecord(h->stage_free.ev, st));
        if (p.capped) MGEA_TRY(launch_clamp_budgets(h->samp_dev, q.lens, q.Tp, B, p.reserve, st));
    } else {
        MGEA_TRY(launch_fill_sampler_params(h->samp_dev, sampler_params(*q.sampler, q.penalty), B, st));
    }
    if (p.kind.scored) {   // the engine's forced-id rows: -1 everywhere, then the caller's [B, n_steps] matrix (steps beyond it stay free)
        const mgea_decoder::Hist hi = h->hist(p.kind.windowed);
        const size_t hs = (size_t)hi.stride;
        MGEA_CHECK_HIP(hipMemsetAsync(hi.forced, 0xff, (size_t)B * hs * sizeof(int32_t), st));
        if (q.forced)
            MGEA_CHECK_HIP(hipMemcpy2DAsync(hi.forced, hs * sizeof(int32_t), q.forced, (size_t)q.n_steps * sizeof(int32_t),
                                            (size_t)q.n_steps * sizeof(int32_t), B, hipMemcpyDeviceToDevice, st));
        MGEA_TRY(mirror_shadow_rows(h, q, p, Mirror::FORCED, st));
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
    GenPlan p;
    MGEA_TRY(plan_generation(q, gen_limits(h), &p));
    // (the conditioning store's [0, len) contract would need its own treatment where the last prompt token is not cached)
    MGEA_REQUIRE(!(causal(h->cfg) && q.sched), MGEA_EINVAL, "decoder_generate_rows_scheduled: MGEA_POS_CAUSAL engines take no prompt schedules");
    mgea_decoder::LastGen last;
    h->last = last;   // a call that fails from here on reports nothing
    MGEA_TRY(gen_prefill(h, q, p, st));
    last.penalized = form_has_presence(p.kind.form);
    last.scheduled = p.kind.scheduled;
    h->last = last;
    if (q.n_steps == 0) return MGEA_OK;
    MGEA_TRY(gen_stage(h, q, p, st));
    int launched = 0;
    MGEA_TRY(gen_run(h, q, p, st, &launched));
    last.graph_replays = launched;
    last.penalized_steps = p.any_penalty ? launched : 0;
    last.biased_steps = p.biased ? launched : 0;
    last.scored_steps = p.kind.scored ? launched : 0;
    last.gram_steps = p.grammar ? launched : 0;
    last.guide_pairs = p.n_pairs;
    last.guide_steps = p.kind.guided ? launched : 0;
    last.sched_steps = p.kind.scheduled ? launched : 0;
    last.trunc_steps = p.truncated ? launched : 0;
    last.trunc_rows = p.truncated ? p.n_trunc : 0;
    last.blend_groups = p.n_groups;
    last.blend_rows = p.n_blend_rows;
    last.blend_steps = p.kind.blended ? launched : 0;
    last.cpen_rows = p.n_cpen;
    last.cpen_steps = p.kind.class_penalized ? launched : 0;
    h->last = last;
    return gen_finish(h, q, p, launched, st);
}

// mgea_decoder_generate and _penalized: the uniform form
int generate_uniform(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp, int32_t n_steps,
                     const mgea_sampler_config* s, float penalty, int32_t* ids_out_dev, void* stream) {
    MGEA_REQUIRE(h && s && prompt_ids_dev && ids_out_dev, MGEA_EINVAL, "decoder_generate: NULL argument");
    MGEA_REQUIRE(std::isfinite(penalty) && penalty > 0.f, MGEA_EINVAL, "decoder_generate: repetition_penalty must be finite and > 0 (got %g)",
                 (double)penalty);
    GenRequest q;
    q.prompt_ids = prompt_ids_dev; q.lens = lens_dev; q.B = B; q.Tp = Tp; q.n_steps = n_steps;
    q.sampler = s; q.penalty = penalty; q.ids_out = ids_out_dev;
    std::lock_guard<std::mutex> lk(h->mu);
    return do_generate(h, q, (hipStream_t)stream);
}

// The mgea_decoder_generate_rows* entry points: what all of them take, then their one prologue.  What the records alone decide
// is checked before the handle is looked at (plan_generation checks it again, with the sampler records).
GenRequest rows_request(const char* who, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp, int32_t n_steps,
                        const mgea_row_sampler* rows, const mgea_row_logits* lrows, int32_t* ids_out_dev) {
    GenRequest q;
    q.who = who;
    q.prompt_ids = prompt_ids_dev; q.lens = lens_dev; q.B = B; q.Tp = Tp; q.n_steps = n_steps;
    q.rows = rows; q.lrows = lrows; q.ids_out = ids_out_dev;
    return q;
}
int generate_rows(mgea_decoder* h, const GenRequest& q, void* stream, bool needs_logprobs = false) {
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
    return generate_rows(h, rows_request("decoder_generate_rows", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, nullptr, ids_out_dev), stream);
}

int mgea_decoder_generate_rows_biased(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      int32_t* ids_out_dev, void* stream) {
    return generate_rows(h, rows_request("decoder_generate_rows", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev), stream);
}

int mgea_decoder_generate_rows_scored(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                      float* choice_logprobs_out_dev, void* stream) {
    GenRequest q = rows_request("decoder_generate_rows_scored", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream, true);
}

int mgea_decoder_generate_rows_grammar(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                       int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                       const int32_t* start_states, const int32_t* forced_ids_dev, int32_t* ids_out_dev,
                                       float* logprobs_out_dev, float* choice_logprobs_out_dev, void* stream) {
    GenRequest q = rows_request("decoder_generate_rows_grammar", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_generate_rows_guided(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      const int32_t* start_states, const mgea_row_guidance* guide, const int32_t* forced_ids_dev,
                                      int32_t* ids_out_dev, float* logprobs_out_dev, float* choice_logprobs_out_dev, void* stream) {
    GenRequest q = rows_request("decoder_generate_rows_guided", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states; q.guide = guide;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_generate_rows_scheduled(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                         int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                         const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                         int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                         float* choice_logprobs_out_dev, void* stream) {
    GenRequest q = rows_request("decoder_generate_rows_scheduled", prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states; q.guide = guide; q.sched = sched; q.n_seg_max = n_seg_max;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_generate_rows_truncated(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                         int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                         const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                         int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                         float* choice_logprobs_out_dev, const mgea_row_truncation* trunc, void* stream) {
    GenRequest q = rows_request(trunc ? "decoder_generate_rows_truncated" : "decoder_generate_rows_scheduled", prompt_ids_dev, lens_dev, B, Tp,
                                n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states; q.guide = guide; q.sched = sched; q.n_seg_max = n_seg_max; q.trunc = trunc;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_generate_rows_blended(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                       int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                       const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                       int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                       float* choice_logprobs_out_dev, const mgea_row_truncation* trunc, const mgea_row_blend* blend,
                                       void* stream) {
    GenRequest q = rows_request(blend   ? "decoder_generate_rows_blended"
                                : trunc ? "decoder_generate_rows_truncated"
                                        : "decoder_generate_rows_scheduled",
                                prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states; q.guide = guide; q.sched = sched; q.n_seg_max = n_seg_max; q.trunc = trunc; q.blend = blend;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_generate_rows_class_penalized(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                               int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                               const int32_t* start_states, const mgea_row_guidance* guide, const mgea_row_schedule* sched,
                                               int32_t n_seg_max, const int32_t* forced_ids_dev, int32_t* ids_out_dev,
                                               float* logprobs_out_dev, float* choice_logprobs_out_dev, const mgea_row_truncation* trunc,
                                               const mgea_row_blend* blend, const mgea_row_class_penalty* cpen, void* stream) {
    GenRequest q = rows_request(cpen    ? "decoder_generate_rows_class_penalized"
                                : blend ? "decoder_generate_rows_blended"
                                : trunc ? "decoder_generate_rows_truncated"
                                        : "decoder_generate_rows_scheduled",
                                prompt_ids_dev, lens_dev, B, Tp, n_steps, rows, logits_rows, ids_out_dev);
    q.start_states = start_states; q.guide = guide; q.sched = sched; q.n_seg_max = n_seg_max; q.trunc = trunc; q.blend = blend; q.cpen = cpen;
    q.forced = forced_ids_dev; q.logprobs_out = logprobs_out_dev; q.choice_out = choice_logprobs_out_dev;
    return generate_rows(h, q, stream);
}

int mgea_decoder_class_penalty_info(mgea_decoder* h, int64_t* out) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_class_penalty_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->cpen_n_class; out[1] = h->last.cpen_rows; out[2] = h->last.cpen_steps;
    return MGEA_OK;
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
        h->cpen_n_class = 0;
    };
    if (!class_of_host) {   // clear
        if (!h->cpen_class) return MGEA_OK;
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
    if (!h->cpen_class) {
        const size_t mb = (size_t)h->cfg.max_batch;
        if (h->dev_cpen.alloc(&h->cpen_class, (size_t)V * sizeof(int32_t)) ||
            h->dev_cpen.alloc(&h->cpen_dev, mb * sizeof(mgea_row_class_penalty)) ||
            h->pinned_cpen.alloc(&h->cpen_stage, mb * sizeof(mgea_row_class_penalty))) {
            clear();
            set_error("decoder_set_penalty_classes: allocation of the class map failed");
            return MGEA_ENOMEM;
        }
        MGEA_CHECK_HIP(hipMemsetAsync(h->cpen_dev, 0, mb * sizeof(mgea_row_class_penalty), st));
    }
    MGEA_CHECK_HIP(hipMemcpyAsync(h->cpen_class, class_of_host, (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // the caller's map is host memory of unknown lifetime
    h->cpen_n_class = n_class;
    return MGEA_OK;
}

int mgea_decoder_blend_info(mgea_decoder* h, int64_t* out) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_blend_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->last.blend_groups; out[1] = h->last.blend_rows; out[2] = h->last.blend_steps;
    return MGEA_OK;
}

int mgea_decoder_truncation_info(mgea_decoder* h, int64_t* out) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_truncation_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->last.trunc_steps; out[1] = h->last.trunc_rows;
    return MGEA_OK;
}

int mgea_decoder_set_grammar(mgea_decoder* h, const int32_t* class_of_host, const int32_t* next_host, int32_t n_state, int32_t n_class,
                             void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder_set_grammar: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    if (n_state == 0) {   // clear
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.form == StepForm::GRAMMAR; });
        h->gram_n_state = h->gram_n_class = 0;
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
    if (n_state != h->gram_n_state || n_class != h->gram_n_class) {
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // a dropped exec may still be replaying
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.form == StepForm::GRAMMAR; });   // their kernel arguments carry the table's shape
    }
    MGEA_CHECK_HIP(hipMemcpyAsync(h->gram_class, class_of_host, (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipMemcpyAsync(h->gram_next, next_host, (size_t)n_state * n_class * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_TRY(launch_grammar_allow(h->gram_next, n_state, n_class, h->gram_allow, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));   // the caller's tables are host memory of unknown lifetime
    h->gram_n_state = n_state;
    h->gram_n_class = n_class;
    h->gram_uploads += 1;
    return MGEA_OK;
}

int mgea_decoder_schedule_info(mgea_decoder* h, int64_t* out, void* stream) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_schedule_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = out[1] = 0;
    if (!h->last.scheduled) return MGEA_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t n = 0;
    MGEA_CHECK_HIP(hipMemcpyAsync(&n, h->cond_switches, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    out[0] = h->last.sched_steps; out[1] = n;
    return MGEA_OK;
}

int mgea_decoder_segments(mgea_decoder* h, int32_t* out_dev, void* stream) {
    MGEA_REQUIRE(h && out_dev, MGEA_EINVAL, "decoder_segments: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_REQUIRE(h->last.scheduled && h->cur_batch > 0, MGEA_EINVAL, "decoder_segments: the last generate() was not scheduled");
    MGEA_CHECK_HIP(hipMemcpyAsync(out_dev, h->cond_cur_seg, (size_t)h->cur_batch * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_guidance_info(mgea_decoder* h, int64_t* out) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_guidance_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->last.guide_pairs; out[1] = h->last.guide_steps;
    return MGEA_OK;
}

int mgea_decoder_set_window(mgea_decoder* h, int32_t sink_pages, int32_t ring_pages, int32_t max_steps, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder_set_window: NULL handle");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    const auto& c = h->cfg;
    auto clear = [&]() {
        h->graphs.drop_if([](const StepGraphs::Key& k) { return k.kind.windowed; });
        h->dev_win.release();
        h->whist = mgea_decoder::Hist{nullptr, nullptr, nullptr, nullptr, 0};
        h->win_S = h->win_R = h->win_max_steps = 0;
    };
    if (sink_pages == 0) {
        if (h->win_S == 0) return MGEA_OK;
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
    if (sink_pages == h->win_S && ring_pages == h->win_R && max_steps == h->win_max_steps) return MGEA_OK;
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    clear();   // the windowed graphs carry S, P and the histories' pointers
    const size_t nhist = (size_t)c.max_batch * (size_t)max_steps;
    DevGroup& g = h->dev_win;
    if (g.alloc(&h->whist.ids, nhist * sizeof(int32_t)) || g.alloc(&h->whist.forced, nhist * sizeof(int32_t)) ||
        g.alloc(&h->whist.lp, nhist * sizeof(float)) || g.alloc(&h->whist.ch, nhist * sizeof(float)) ||
        g.alloc(&h->win_evict, (size_t)c.max_batch * sizeof(int32_t))) {
        clear();
        set_error("decoder_set_window: allocation of the histories for max_steps %d failed", max_steps);
        return MGEA_ENOMEM;
    }
    MGEA_CHECK_HIP(hipMemsetAsync(h->win_evict, 0, (size_t)c.max_batch * sizeof(int32_t), st));
    h->whist.stride = max_steps;
    h->win_S = sink_pages; h->win_R = ring_pages; h->win_max_steps = max_steps;
    return MGEA_OK;
}

int mgea_decoder_window_info(mgea_decoder* h, int32_t* out, int32_t* evictions_out, void* stream) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_window_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->win_S; out[1] = h->win_R; out[2] = h->win_max_steps;
    if (evictions_out) {
        MGEA_REQUIRE(h->win_S > 0, MGEA_EINVAL, "decoder_window_info: no window is set");
        hipStream_t st = (hipStream_t)stream;
        const int B = h->cur_batch > 0 ? h->cur_batch : 0;
        MGEA_CHECK_HIP(hipMemcpyAsync(evictions_out, h->win_evict, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
    }
    return MGEA_OK;
}

int mgea_decoder_grammar_states(mgea_decoder* h, int32_t* out_dev, void* stream) {
    MGEA_REQUIRE(h && out_dev, MGEA_EINVAL, "decoder_grammar_states: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    MGEA_CHECK_HIP(hipMemcpyAsync(out_dev, h->gram_state, (size_t)(h->cur_batch > 0 ? h->cur_batch : 0) * sizeof(int32_t),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_decoder_grammar_info(mgea_decoder* h, int64_t* out) {
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_grammar_info: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->gram_n_state; out[1] = h->gram_n_class; out[2] = h->gram_uploads; out[3] = h->last.gram_steps;
    return MGEA_OK;
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
    MGEA_REQUIRE(h && out, MGEA_EINVAL, "decoder_stats: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    // the ABI's order (include/mgea.h), written down here and nowhere else
    out[0] = h->n.graph_nodes;
    out[1] = h->last.graph_replays;
    out[2] = h->graphs.inserted();        // graph_instantiates: lifetime captures + instantiations
    out[3] = h->last.scored_steps;
    out[4] = (int64_t)h->graphs.size();   // graphs_cached
    out[5] = h->n.prefill16_forwards;
    out[6] = h->last.penalized_steps;
    out[7] = h->last.biased_steps;
    return MGEA_OK;
}

}  // extern "C"
