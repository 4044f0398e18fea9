// The decoder handle: what mgea_decoder owns, its accessors and predicates, and the few functions its two translation units share --
// decoder.hip (the engine: forward, step, graphs, create) and decoder_generate.hip (generate(), the per-feature setters and readers).
#pragma once
#include <mutex>
#include <vector>

#include "common.h"
#include "devmem.h"
#include "hipres.h"
#include "rowtable.h"

#pragma GCC visibility push(hidden)   // nothing here is part of the library's ABI
namespace mgea {
enum { T_TOK = 0, T_POS = 1, L_LN1W = 0, L_LN1B, L_INW, L_INB, L_OUTW, L_OUTB, L_LN2W, L_LN2B, L_FC1W, L_FC1B,
       L_FC2W, L_FC2B, L_COUNT };
// "use true positions": both modes that are not the reference's (every site that adds a position asks here)
inline bool true_positions(const mgea_decoder_config& c) { return c.pos_mode == MGEA_POS_ABSOLUTE || c.pos_mode == MGEA_POS_CAUSAL; }
inline bool causal(const mgea_decoder_config& c) { return c.pos_mode == MGEA_POS_CAUSAL; }
}  // namespace mgea
#pragma GCC visibility pop

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
    mgea::DevGroup dev;            // handle state: mgea_decoder_create and build_tiled_weights, until destroy
    mgea::DevGroup dev_ws;         // the workspace: released and regrown by ensure_ws
    mgea::DevGroup dev_p16_rows;   // Prefill16's activations and tables, regrown with its row count (ensure_p16)
    mgea::DevGroup dev_p16_mats;   // Prefill16's matrices p16.w / p16.vec, kept across refresh_weights
    mgea::DevGroup dev_win;        // the KV window's histories and eviction counters: mgea_decoder_set_window, until the window changes
    mgea::DevGroup dev_cond;       // the conditioning store, the rows' schedules and segments: scheduled generations only (ensure_cond)
    mgea::DevGroup dev_cpen;       // the penalty class map and the rows' class-penalty records: mgea_decoder_set_penalty_classes, until it is cleared
    // The handle's other HIP resources, declared behind the device groups, so that they go first (members die in reverse order):
    // the graphs, the pinned staging arrays and the events, then the device memory.
    mgea::Event stage_free;        // recorded after the uploads of gen_stage: the tables' pinned stages may be rewritten once it has completed
    mgea::PinnedGroup pinned;      // the stages of the tables allocated at create
    mgea::PinnedGroup pinned_cond; // cond.sched's stage: with dev_cond
    mgea::PinnedGroup pinned_cpen; // cpen.rec's stage: with dev_cpen

    // KV pool
    mgea::KvPool kv{};
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
    // structure lives in device memory (per-row state, page table, presence bitmaps, and the rows' sampler records in samp.dev), so a
    // request with a new seed / temperature / top-k / top-p / EOS id / repetition penalty / budget -- or a batch whose rows differ in
    // them -- replays an existing graph: no capture, no instantiate.
    mgea::StepGraphs graphs;
    // The rows' records reach the device through RowTables (rowtable.h): gen_stage fills the pinned stages, mirrors the rows that run on
    // another row's inputs and uploads rows [0, B) in stream order, between the wait for stage_free and its record.  The graphs hold
    // the tables' device pointers, so a request with other values replays them.
    mgea::RowTable<mgea::SamplerParams> samp;          // one sampler record per row (common.h), staged by mgea_decoder_generate_rows*
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
    struct Hist { int32_t* ids; int32_t* forced; float* lp; float* ch; int stride; };
    // The KV window (mgea_decoder_set_window; the contract: include/mgea.h).  S > 0: every generation keeps P = S + R pages per row --
    // the sink and a ring -- and each of its steps opens with the evict launch (kv_window.hip), so it may run max_steps steps whatever
    // max_ctx is.  Its id, forced-id and log-probability histories are therefore a second set, hist, with stride max_steps, next to the
    // rows' eviction counters evict [max_batch] in dev_win: allocated by set_window and by nothing else, so an engine without a window
    // allocates what it always did.  "Windowed" is part of the step-graph key; changing the window drops those graphs alone.
    // dirty: a windowed generation has run since the last reset -- ctx_len counts cached tokens, the host mirror (host_max_len) no longer
    // says what the rows hold, and mgea_decoder_step / an extending forward are refused.
    struct Window { int S = 0, R = 0, max_steps = 0; bool dirty = false; int32_t* evict = nullptr; Hist hist{nullptr, nullptr, nullptr, nullptr, 0}; } win;
    Hist hist(bool windowed) const { return windowed ? win.hist : Hist{ids_hist, forced, lp_hist, ch_hist, ids_hist_stride}; }
    int32_t* err_flag = nullptr;   // sticky device flags (bit 0: a token id outside the vocabulary was clamped; bit 1: a forced id was banned by the grammar)
    // Token grammar (mgea_decoder_set_grammar; GrammarArgs, common.h): one automaton per engine.  The tables live in buffers of their
    // largest size, allocated at create behind the other sampler buffers, so the GRAMMAR graphs hold stable pointers whatever table is
    // uploaded; the shape travels in the graphs' kernel arguments, so an upload of another shape drops those graphs.  state: the rows'
    // states on the device, staged from the call's start states before the first step.
    struct Grammar {
        int32_t *class_of = nullptr, *next = nullptr; uint32_t* allow = nullptr;
        mgea::RowTable<int32_t> state;
        int n_state = 0, n_class = 0; int64_t uploads = 0;
    } gram;
    // Classifier-free guidance (mgea_decoder_generate_rows_guided; guidance.hip): the shadow row of every conditional row (-1 elsewhere)
    // and its scale, allocated at create behind the grammar's buffers
    struct Guidance { mgea::RowTable<int32_t> partner{mgea::RowTableBase::OWN}; mgea::RowTable<float> scale{mgea::RowTableBase::OWN}; } guide;
    // Truncation (mgea_decoder_generate_rows_truncated; TruncArgs, common.h): the rows' min-p / typical-p / epsilon / eta records,
    // allocated at create behind the guidance vectors
    struct Truncation { mgea::RowTable<mgea_row_truncation> rec; } trunc;
    // Emotion blends (mgea_decoder_generate_rows_blended; blend.hip): every row's group leader (-1 = in no group) and its weight,
    // allocated at create behind the truncation records
    struct Blend { mgea::RowTable<int32_t> leader{mgea::RowTableBase::OWN}; mgea::RowTable<float> weight{mgea::RowTableBase::OWN}; } blend;
    // Windowed penalties over token classes (mgea_decoder_generate_rows_class_penalized; class_penalty.hip).  Everything here belongs to
    // dev_cpen / pinned_cpen and is allocated by mgea_decoder_set_penalty_classes, never by create: class_of [vocab] the map (values in
    // [-1, n_class)), rec the rows' records, staged per call: a request with other values or windows replays the class-penalised graphs.
    struct ClassPenalty { int32_t* class_of = nullptr; mgea::RowTable<mgea_row_class_penalty> rec; int n_class = 0; } cpen;
    // Emotion transitions (mgea_decoder_generate_rows_scheduled; recondition.hip).  Everything here belongs to dev_cond / pinned_cond and is
    // allocated by the first scheduled call, never by create: store holds the K | V of positions [0, len_b) of every prompt variant (bytes
    // of it; a call that needs more synchronises, drops the scheduled graphs and regrows the whole group), sched the rows' records,
    // cur_seg [max_batch] their segments, switches [1] the call's switch count, meta [4] / len [max_batch] the store's layout words and
    // the rows' prompt lengths (written by the gather kernel).
    struct Cond {
        void* store = nullptr; int64_t bytes = 0;
        mgea::RowTable<mgea_row_schedule> sched{mgea::RowTableBase::OWN};   // (a shadow row has one segment whatever its conditional row has)
        int32_t *cur_seg = nullptr, *switches = nullptr, *meta = nullptr, *len = nullptr;
    } cond;
    mgea::AttnSplit attn_split{};        // scratch of the split-context decode attention (small batches; attn_paged.hip)
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
    // What the last generate() did; the _info and stats entry points derive their figures from it.  do_generate assigns it whole: zeroed
    // once the call is planned, the flags once its prefill is through, the plan and the step count once its steps have run.
    struct LastGen {
        bool penalized = false;   // it applied a penalty (or a bias): presence holds its rows
        bool scheduled = false;   // it was scheduled: cond.cur_seg / cond.switches hold its rows
        mgea::GenPlan plan{};
        int64_t launched = 0;     // the decode steps that ran
        int64_t steps(bool on) const { return on ? launched : 0; }   // ... of a generation whose plan says `on`
    } last;
    // what mgea_decoder_stats reports of the handle's lifetime, besides the graph cache's own two figures
    struct Counters { int64_t graph_nodes = 0, prefill16_forwards = 0; } n;
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg)
    int prof_stride = 0;  // 0 = off; n = time every n-th decode step of generate(), run eagerly
    bool prof_now = false;
    struct ProfRec { mgea::Event a, b; int cls; };
    std::vector<ProfRec> prof;   // unread records go with the handle

    const float* w(int idx) const { return arena + off[idx]; }
    const float* lw(int layer, int j) const { return arena + off[2 + layer * mgea::L_COUNT + j]; }
    const float* head_w() const { return arena + off[2 + cfg.n_layer * mgea::L_COUNT]; }
    const float* head_b() const { return arena + off[3 + cfg.n_layer * mgea::L_COUNT]; }
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

#pragma GCC visibility push(hidden)
namespace mgea {

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

// Fused path for M = B*T <= MGEA_FUSED_MAX_ROWS rows in the KV-cache block mode: 5 launches per layer
// (gemm_skinny.hip); x carries per-row LayerNorm partial statistics between kernels.
inline bool fused_geometry(const mgea_decoder_config& c) {
    return c.block_mode == MGEA_BLOCK_PRELN_GELU && (c.d_model % 128) == 0 && c.d_model >= 256 && c.d_model <= 1024;
}
inline bool fused_ok(const mgea_decoder* h, int M) {
    return fused_geometry(h->cfg) && M <= MGEA_FUSED_MAX_ROWS && M <= h->ws_tokens && !h->force_unfused && h->wt;
}

// single-token decode steps of <= 2 rows (the reference's serving case is B = 1): wave-level dot products on the
// row-major arena weights instead of 16 x 16 MFMA tiles (gemv_small.hip)
inline bool gemv_ok(const mgea_decoder* h, int M, int T, const int32_t* lens, bool use_cache_attn) {
    const auto& c = h->cfg;
    return !h->no_gemv && !h->f16 && T == 1 && !lens && use_cache_attn && gemv_shape_ok(M, c.d_model, c.d_model) &&
           gemv_shape_ok(M, c.d_model, c.d_ff);
}

// The KV pool as a launch that may compute page ids sees it: switch attn_arith_pages off sends every page id through the table
inline KvPool kv_view(const mgea_decoder* h) {
    KvPool pool = h->kv;
    if (!tune(TUNE_ATTN_ARITH_PAGES)) pool.arith_batch = 0;
    return pool;
}

// decoder.hip, for decoder_generate.hip (the caller holds h->mu)
int ensure_ws(mgea_decoder* h, int64_t M);
int do_reset(mgea_decoder* h, int B, int max_len, hipStream_t st);
int do_forward(mgea_decoder* h, const int32_t* ids, const int32_t* lens, int B, int T, float* logits_out, hipStream_t st);
int qkv0_path(const mgea_decoder* h, int B);
int ensure_qkv0(mgea_decoder* h, int path, hipStream_t st);
int enqueue_gen_step(mgea_decoder* h, int B, const StepKind& kind, hipStream_t st);
int prime_gen(mgea_decoder* h, int B, hipStream_t st);
int step_graph(mgea_decoder* h, int B, const StepKind& kind, int steps, hipStream_t st, hipGraphExec_t* out);

}  // namespace mgea
#pragma GCC visibility pop
