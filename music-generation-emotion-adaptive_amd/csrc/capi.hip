// C-ABI glue: error string, device probe, LoRA fold and the op-level entry points the parity
// tests use to check each kernel against the oracle in isolation (include/mgea.h).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "devmem.h"
#include "hipres.h"
#include "rowtable.h"

namespace mgea {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

bool dev_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
void dev_free(void* p) { (void)hipFree(p); }
bool pinned_malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, 0) == hipSuccess; }
void pinned_free(void* p) { (void)hipHostFree(p); }
int upload_async(void* dst, const void* src, size_t bytes, hipStream_t st) {
    MGEA_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return MGEA_OK;
}
void event_destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
void graph_destroy(hipGraph_t graph, hipGraphExec_t exec) {
    if (exec) (void)hipGraphExecDestroy(exec);   // (NULL: a graph whose capture or instantiation failed)
    if (graph) (void)hipGraphDestroy(graph);
}

// ---- switches: one table, initialised from the environment when the library is loaded ---------
namespace {
struct TuneEntry { int key; const char* name; const char* env; int dflt; };
// (each row names its key: the table is looked up by key, never by position)
const TuneEntry kTune[] = {
    {TUNE_BF16_GEMM_TILE, "bf16_gemm_tile", "MGEA_BF16_GEMM_TILE", 0},
    {TUNE_BF16_GEMM_SMALL, "bf16_gemm_small", "MGEA_BF16_GEMM_SMALL", 0},
    {TUNE_BF16_GEMM_TAIL, "bf16_gemm_tail", "MGEA_BF16_GEMM_TAIL", 2},
    {TUNE_BF16_GEMM_PHASES, "bf16_gemm_phases", "MGEA_BF16_GEMM_PHASES", 2},
    {TUNE_BF16_GEMM_REVERSE, "bf16_gemm_reverse", "MGEA_BF16_GEMM_REVERSE", 1},
    {TUNE_BERT_BF16_NOFOLD, "bert_bf16_nofold", "MGEA_BERT_BF16_NOFOLD", 0},
    {TUNE_DECODER_PREFILL_FULL, "decoder_prefill_full", "MGEA_DECODER_PREFILL_FULL", 0},
    {TUNE_BERT_FULL_LAST_LAYER, "bert_full_last_layer", "MGEA_BERT_FULL_LAST_LAYER", 0},
    {TUNE_DECODER_UNFUSED, "decoder_unfused", "MGEA_DECODER_UNFUSED", 0},
    {TUNE_DECODER_NOGEMV, "decoder_nogemv", "MGEA_DECODER_NOGEMV", 0},
    {TUNE_DECODER_NOGRAPH, "decoder_nograph", "MGEA_DECODER_NOGRAPH", 0},
    {TUNE_ATTN16_WIDE, "attn16_wide", "MGEA_ATTN16_WIDE", 1},
    {TUNE_DECODER_PREFILL16_PAGES, "decoder_prefill16_pages", "MGEA_DECODER_PREFILL16_PAGES", 1},
    {TUNE_DECODER_PREFILL16, "decoder_prefill16", "MGEA_DECODER_PREFILL16", 1},
    {TUNE_HEAD_BALANCED, "head_balanced", "MGEA_HEAD_BALANCED", 1},
    {TUNE_ATTN16_PIPE, "attn16_pipe", "MGEA_ATTN16_PIPE", 1},
    {TUNE_SKINNY_ONE_PER_CU, "skinny_one_per_cu", "MGEA_SKINNY_ONE_PER_CU", 0},
    {TUNE_SAMPLER_WAVE_SELECT, "sampler_wave_select", "MGEA_SAMPLER_WAVE_SELECT", 1},
    {TUNE_ATTN_SPLIT, "attn_split", "MGEA_ATTN_SPLIT", 64},
    {TUNE_DECODER_GRAPH_STEPS, "decoder_graph_steps", "MGEA_DECODER_GRAPH_STEPS", 8},
    {TUNE_ATTN_ARITH_PAGES, "attn_arith_pages", "MGEA_ATTN_ARITH_PAGES", 1},
    {TUNE_DECODER_QKV0_TABLE, "decoder_qkv0_table", "MGEA_DECODER_QKV0_TABLE", 1},
    {TUNE_ATTN_CAUSAL_WALK, "attn_causal_walk", "MGEA_ATTN_CAUSAL_WALK", 1},
};
static_assert(sizeof(kTune) / sizeof(kTune[0]) == TUNE_COUNT, "one table row per switch");
std::atomic<int> g_tune[TUNE_COUNT];
struct TuneInit {
    TuneInit() {
        for (const TuneEntry& t : kTune) {
            const char* e = getenv(t.env);
            g_tune[t.key].store(e && e[0] ? atoi(e) : t.dflt, std::memory_order_relaxed);
        }
    }
} g_tune_init;
int tune_index(const char* name) {
    for (const TuneEntry& t : kTune)
        if (name && !strcmp(name, t.name)) return t.key;
    return -1;
}
}  // namespace
int tune(int key) { return g_tune[key].load(std::memory_order_relaxed); }

int device_info(DeviceInfo* out) {
    static std::mutex mu;
    static int n_cu[64] = {0};
    int dev = 0;
    MGEA_CHECK_HIP(hipGetDevice(&dev));
    MGEA_REQUIRE(dev >= 0 && dev < 64, MGEA_EINVAL, "device id %d out of range", dev);
    std::lock_guard<std::mutex> lk(mu);
    if (!n_cu[dev]) {
        hipDeviceProp_t prop;
        MGEA_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
        n_cu[dev] = prop.multiProcessorCount;
    }
    out->dev = dev;
    out->n_cu = n_cu[dev];
    return MGEA_OK;
}
int set_max_dynamic_lds(const void* fn, int bytes, int dev, uint64_t* done) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (*done >> dev & 1) return MGEA_OK;
    MGEA_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    *done |= (uint64_t)1 << dev;
    return MGEA_OK;
}
}  // namespace mgea

using namespace mgea;

// a sampler launch on caller buffers: no fused tail, the host's step index
static SampleCall op_sample_call(const float* logits_dev, int B, int V, int64_t step, int32_t* ids_out_dev, float* probs_out_dev) {
    SampleCall c{};
    c.logits = logits_dev; c.B = B; c.V = V; c.step_host = step; c.ids_out = ids_out_dev; c.probs_out = probs_out_dev;
    return c;
}

// The temporaries of one rows launch (mgea_op_sample_rows*, kind 4 of mgea_op_step_tail): the rows' device records, their bias rows
// (row b at b * V; rows without one are never read), the grammar's allow bitmask, the truncation records, and an all-zero presence
// bitmap where a grammar or a truncating launch got none from the caller (both forms are built on the PENALTY one).  The group frees
// them on return; the caller synchronises the stream first.  The callers keep their own argument checks and return codes.
struct RowsStage {
    SamplerParams* rec_dev = nullptr;
    float* bias_dev = nullptr;
    uint32_t *allow_dev = nullptr, *pres_tmp = nullptr;
    mgea_row_truncation* trunc_dev = nullptr;
    DevGroup tmp;   // (declared after the pointers it fills)
    hipError_t hip_err = hipSuccess;   // fill(): the enqueue that failed

    enum { RECORDS = 1, BIAS, GRAMMAR, TRUNC };
    static const char* what(int bad) { return bad == RECORDS ? "records" : bad == BIAS ? "bias rows" : bad == GRAMMAR ? "grammar's bitmask" : "truncation records"; }
    // Allocates, in this order and before anything is enqueued: records, bias rows, allow bitmask, truncation records, the stand-in
    // bitmap.  0, or which allocation failed.
    int alloc(int B, int V, bool records, bool bias, const GrammarArgs* g, bool trunc, bool caller_bitmap) {
        const size_t np = (size_t)B * presence_words(V) * sizeof(uint32_t);
        if (records && tmp.alloc(&rec_dev, (size_t)B * sizeof(SamplerParams)) != MGEA_OK) return RECORDS;
        if (bias && tmp.alloc(&bias_dev, (size_t)B * V * sizeof(float)) != MGEA_OK) return BIAS;
        if (g && (tmp.alloc(&allow_dev, (size_t)g->n_state * grammar_words(g->n_class) * sizeof(uint32_t)) != MGEA_OK ||
                  (!caller_bitmap && tmp.alloc(&pres_tmp, np) != MGEA_OK)))
            return GRAMMAR;
        if (trunc && (tmp.alloc(&trunc_dev, (size_t)B * sizeof(mgea_row_truncation)) != MGEA_OK ||
                      (!caller_bitmap && !pres_tmp && tmp.alloc(&pres_tmp, np) != MGEA_OK)))
            return TRUNC;
        return 0;
    }
    // Enqueues what fills them -- records, allow bitmask (its own kernel), truncation records, the zeroed bitmap, the bias rows of
    // lrows (device-to-device, one copy per row that has one) -- stopping at the first failure, and writes them into c.  MGEA_OK,
    // launch_grammar_allow's code, or MGEA_EHIP with hip_err set.
    int fill(SampleCall& c, int B, int V, const SamplerParams* rec, const mgea_row_logits* lrows, const GrammarArgs* g,
             const mgea_row_truncation* trunc, hipStream_t st) {
        c.params_dev = rec_dev;   // every scalar comes from the records
        c.bias = bias_dev;
        if (pres_tmp) c.presence = pres_tmp;
        if (rec_dev && (hip_err = hipMemcpyAsync(rec_dev, rec, (size_t)B * sizeof(SamplerParams), hipMemcpyHostToDevice, st)) != hipSuccess) return MGEA_EHIP;
        if (g) {
            c.grammar = *g;
            c.grammar.allow = allow_dev;
            c.grammar.words = grammar_words(g->n_class);
            MGEA_TRY(launch_grammar_allow(g->next, g->n_state, g->n_class, allow_dev, st));
        }
        if (trunc) {
            c.trunc = TruncArgs{trunc_dev};
            if ((hip_err = hipMemcpyAsync(trunc_dev, trunc, (size_t)B * sizeof(mgea_row_truncation), hipMemcpyHostToDevice, st)) != hipSuccess) return MGEA_EHIP;
        }
        if (pres_tmp && (hip_err = hipMemsetAsync(pres_tmp, 0, (size_t)B * presence_words(V) * sizeof(uint32_t), st)) != hipSuccess) return MGEA_EHIP;
        for (int b = 0; lrows && b < B; ++b)
            if (lrows[b].bias_dev && (hip_err = hipMemcpyAsync(bias_dev + (size_t)b * V, lrows[b].bias_dev, (size_t)V * sizeof(float),
                                                               hipMemcpyDeviceToDevice, st)) != hipSuccess)
                return MGEA_EHIP;
        return MGEA_OK;
    }
};

// mgea_op_sample_rows(_biased, _scored): the rows' records and bias vectors to device memory, one sampler launch (defined at the end)
static int op_sample_rows(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                          const mgea_row_logits* lrows, int64_t step, int32_t* ids_out_dev, float* probs_out_dev, const ScoreArgs& score,
                          void* stream, const GrammarArgs* grammar = nullptr, const mgea_row_truncation* trunc = nullptr);

extern "C" {

const char* mgea_last_error(void) { return get_error(); }
int mgea_version(void) { return 100; }

int mgea_tune_set(const char* name, int32_t value) {
    const int i = tune_index(name);
    MGEA_REQUIRE(i >= 0, MGEA_EINVAL, "tune_set: unknown switch '%s'", name ? name : "(null)");
    g_tune[i].store(value, std::memory_order_relaxed);
    return MGEA_OK;
}
int mgea_tune_get(const char* name, int32_t* value_out) {
    const int i = tune_index(name);
    MGEA_REQUIRE(i >= 0 && value_out, MGEA_EINVAL, "tune_get: unknown switch '%s'", name ? name : "(null)");
    *value_out = tune(i);
    return MGEA_OK;
}

int mgea_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        set_error("hipGetDeviceCount failed: no HIP device visible");
        return MGEA_ENODEVICE;
    }
    return n;
}

int mgea_lora_merge(float* w_dev, const float* a_dev, const float* b_dev, int32_t out_dim, int32_t in_dim, int32_t r,
                    float scale, void* stream) {
    MGEA_REQUIRE(w_dev && a_dev && b_dev && out_dim > 0 && in_dim > 0 && r > 0, MGEA_EINVAL, "lora_merge: bad argument");
    return launch_lora_merge(w_dev, a_dev, b_dev, out_dim, in_dim, r, scale, (hipStream_t)stream);
}

int64_t mgea_op_gemm_workspace_floats(int32_t M, int32_t N, int32_t split_k) {
    if (split_k < 1) split_k = 1;
    return (int64_t)split_k * slab_floats(M, N);
}

int mgea_op_gemm_f32(const float* a_dev, const float* w_dev, const float* bias_dev, float* out_dev, int32_t M,
                     int32_t N, int32_t K, int32_t split_k, float* workspace_dev, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev && workspace_dev, MGEA_EINVAL, "op_gemm: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (split_k <= 0) split_k = M > 64 ? 1 : pick_split_k(M, N, K);   // the caller sized the workspace for this (mgea.h)
    const int S = launch_gemm_f32(a_dev, K, w_dev, K, workspace_dev, M, N, K, split_k, st);
    if (S < 0) return S;
    return launch_bias_act(workspace_dev, S, slab_floats(M, N), (int)slab_ld(N), bias_dev, out_dev, N, M, N, ACT_NONE, st);
}

int mgea_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int32_t M, int32_t C,
                      float eps, void* stream) {
    MGEA_REQUIRE(x_dev && w_dev && b_dev && y_dev, MGEA_EINVAL, "op_layernorm: NULL argument");
    return launch_layernorm(x_dev, w_dev, b_dev, y_dev, M, C, eps, (hipStream_t)stream);
}

int mgea_op_attention_f32(const float* qkv_dev, const int32_t* lens_dev, const int32_t* mask_dev, float* out_dev,
                          int32_t B, int32_t T, int32_t n_head, int32_t head_dim, void* stream) {
    MGEA_REQUIRE(qkv_dev && out_dev, MGEA_EINVAL, "op_attention: NULL argument");
    return launch_attn_dense(qkv_dev, lens_dev, mask_dev, out_dev, B, T, n_head, head_dim, 0, (hipStream_t)stream);
}

int mgea_op_attention_f32_ex(const float* qkv_dev, const int32_t* lens_dev, const int32_t* mask_dev, const int32_t* cu_seqlens_dev,
                             float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim, int32_t tiled_out, void* stream) {
    MGEA_REQUIRE(qkv_dev && out_dev, MGEA_EINVAL, "op_attention: NULL argument");
    // (cu with lens / mask / tiled_out is the launcher's refusal; here only what keeps a k-tiled out inside the size mgea.h documents)
    MGEA_REQUIRE(!tiled_out || cu_seqlens_dev || ((int64_t)B * T <= MGEA_FUSED_MAX_ROWS && ((n_head * head_dim) % 32 == 0 || (int64_t)B * T <= 64)),
                 MGEA_EINVAL, "op_attention: a k-tiled out holds at most %d rows (64 when its width is no multiple of 32)", MGEA_FUSED_MAX_ROWS);
    return launch_attn_dense(qkv_dev, lens_dev, mask_dev, out_dev, B, T, n_head, head_dim, tiled_out != 0, (hipStream_t)stream, cu_seqlens_dev);
}

int mgea_op_attention_f32_causal(const float* qkv_dev, const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head,
                                 int32_t head_dim, int32_t tiled_out, void* stream) {
    MGEA_REQUIRE(qkv_dev && out_dev, MGEA_EINVAL, "op_attention: NULL argument");
    MGEA_REQUIRE(!tiled_out || ((int64_t)B * T <= MGEA_FUSED_MAX_ROWS && ((n_head * head_dim) % 32 == 0 || (int64_t)B * T <= 64)),
                 MGEA_EINVAL, "op_attention: a k-tiled out holds at most %d rows (64 when its width is no multiple of 32)", MGEA_FUSED_MAX_ROWS);
    return launch_attn_dense(qkv_dev, lens_dev, nullptr, out_dev, B, T, n_head, head_dim, tiled_out != 0, (hipStream_t)stream, nullptr, 1);
}

int mgea_op_logprob_gather(const float* logits_dev, int64_t ld, const int32_t* targets_dev, float* out_dev, int32_t M, int32_t V,
                           void* stream) {
    return launch_logprob_gather(logits_dev, ld, targets_dev, out_dev, M, V, (hipStream_t)stream);
}

int mgea_op_f32_to_bf16(const float* src_dev, void* dst_dev, int64_t n, void* stream) {
    MGEA_REQUIRE(src_dev && dst_dev && n > 0, MGEA_EINVAL, "op_f32_to_bf16: bad argument");
    return launch_f32_to_bf16(src_dev, dst_dev, n, (hipStream_t)stream);
}

int mgea_op_gemm_bf16(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* out_dev,
                      int32_t M, int32_t N, int32_t K, int32_t epi, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev, MGEA_EINVAL, "op_gemm_bf16: NULL argument");
    return launch_gemm_bf16(a_dev, K, w_dev, K, bias_dev, res_dev, out_dev, N, M, N, K, epi, (hipStream_t)stream);
}

int mgea_op_gemm_bf16_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* out_dev,
                         int32_t M, int32_t N, int32_t K, int32_t epi, const float* rowstat_dev, const float* c1_dev,
                         const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev, MGEA_EINVAL, "op_gemm_bf16_ln: NULL argument");
    const BfEpiLn ln{rowstat_dev, c1_dev, ln_g_dev, ln_b_dev, stats_out_dev};
    GemmBf16Info gi{-1, 0};
    const int rc = launch_gemm_bf16(a_dev, K, w_dev, K, bias_dev, res_dev, out_dev, N, M, N, K, epi, (hipStream_t)stream, &gi,
                                    epi >= BEPI_LNFOLD ? &ln : nullptr);
    if (info_out) { info_out[0] = gi.kernel; info_out[1] = gi.half_tiles; }
    return rc;
}

int mgea_op_ln_rowstat(const float* part_dev, float* rowstat_dev, int32_t M, int32_t n_part, int32_t C, float eps, void* stream) {
    MGEA_REQUIRE(part_dev && rowstat_dev && M > 0 && n_part > 0 && C > 0 && C % n_part == 0, MGEA_EINVAL, "op_ln_rowstat: bad argument");
    return launch_ln_rowstat(part_dev, rowstat_dev, M, n_part, C, eps, (hipStream_t)stream);
}

int mgea_op_fold_ln_bf16(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                         void* wf_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream) {
    MGEA_REQUIRE(w_dev && gamma_dev && beta_dev && bias_dev && wf_out_dev && c1_out_dev && c2_out_dev && N > 0 && K > 0, MGEA_EINVAL,
                 "op_fold_ln_bf16: bad argument");
    return launch_fold_ln_weights_bf16(w_dev, gamma_dev, beta_dev, bias_dev, wf_out_dev, c1_out_dev, c2_out_dev, N, K, (hipStream_t)stream);
}

int mgea_op_attention_bf16(const void* qkv_dev, const int32_t* mask_dev, void* out_dev, int32_t B, int32_t T,
                           int32_t n_head, int32_t head_dim, void* stream) {
    MGEA_REQUIRE(qkv_dev && out_dev, MGEA_EINVAL, "op_attention_bf16: NULL argument");
    return launch_attn_bf16(qkv_dev, mask_dev, out_dev, B, T, n_head, head_dim, (hipStream_t)stream);
}

int mgea_op_layernorm_bf16(const void* x_dev, const float* w_dev, const float* b_dev, void* y_dev, int32_t M, int32_t C,
                           float eps, void* stream) {
    MGEA_REQUIRE(x_dev && w_dev && b_dev && y_dev, MGEA_EINVAL, "op_layernorm_bf16: NULL argument");
    return launch_layernorm_bf16(x_dev, w_dev, b_dev, y_dev, M, C, eps, (hipStream_t)stream);
}

// ---- the 16-bit kernels of the fp16 decoder and the paged attention, one kernel per call (tests) ----
// one layer of KV pages on a caller buffer (mgea.h)
static KvPool op_pool(const void* pages_dev, int n_pages, int H, int dh, int f16, int arith_batch) {
    KvPool p{};
    p.base = const_cast<void*>(pages_dev); p.n_pages = n_pages; p.H = H; p.dh = dh;
    p.layer_stride = (int64_t)n_pages * 2 * H * MGEA_KV_PAGE_TOKENS * dh;
    p.f16 = f16; p.arith_batch = arith_batch;
    return p;
}

int mgea_op_gemm_f16_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* out_dev,
                        int32_t M, int32_t N, int32_t K, int32_t epi, const float* rowstat_dev, const float* c1_dev,
                        const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev, MGEA_EINVAL, "op_gemm_f16_ln: NULL argument");
    const BfEpiLn ln{rowstat_dev, c1_dev, ln_g_dev, ln_b_dev, stats_out_dev};
    GemmBf16Info gi{-1, 0};
    const int rc = launch_gemm_bf16(a_dev, K, w_dev, K, bias_dev, res_dev, out_dev, N, M, N, K, epi, (hipStream_t)stream, &gi, &ln, 1);
    if (info_out) { info_out[0] = gi.kernel; info_out[1] = gi.half_tiles; }
    return rc;
}

int mgea_op_gemm16(const void* a_dev, int32_t lda, const void* w_dev, int32_t ldw, const float* bias_dev, const void* res_dev, void* out_dev,
                   int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t f16, int32_t reverse, const float* rowstat_dev,
                   const float* c1_dev, const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev, MGEA_EINVAL, "op_gemm16: NULL argument");
    MGEA_REQUIRE(lda >= K && ldw >= K && ldc >= N, MGEA_EINVAL, "op_gemm16: lda %d / ldw %d below K = %d or ldc %d below N = %d", lda, ldw, K, ldc, N);
    const BfEpiLn ln{rowstat_dev, c1_dev, ln_g_dev, ln_b_dev, stats_out_dev};
    GemmBf16Info gi{-1, 0, 0};
    const int rc = launch_gemm_bf16(a_dev, lda, w_dev, ldw, bias_dev, res_dev, out_dev, ldc, M, N, K, epi, (hipStream_t)stream, &gi,
                                    epi >= BEPI_LNFOLD ? &ln : nullptr, f16 != 0, reverse != 0);
    if (info_out) { info_out[0] = gi.kernel; info_out[1] = gi.half_tiles; info_out[2] = gi.tail_mode; }
    return rc;
}

int mgea_op_f32_to_16(const float* src_dev, void* dst_dev, int64_t n, int32_t dtype, void* stream) {
    MGEA_REQUIRE(src_dev && dst_dev && n > 0 && (dtype == MGEA_DTYPE_BF16 || dtype == MGEA_DTYPE_F16), MGEA_EINVAL, "op_f32_to_16: bad argument");
    return launch_f32_to_bf16(src_dev, dst_dev, n, (hipStream_t)stream, dtype == MGEA_DTYPE_F16);
}

int mgea_op_fold_ln_16(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                       int32_t dtype, void* wf_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream) {
    MGEA_REQUIRE(w_dev && gamma_dev && beta_dev && bias_dev && wf_out_dev && c1_out_dev && c2_out_dev && N > 0 && K > 0 &&
                     (dtype == MGEA_DTYPE_BF16 || dtype == MGEA_DTYPE_F16),
                 MGEA_EINVAL, "op_fold_ln_16: bad argument");
    return launch_fold_ln_weights_bf16(w_dev, gamma_dev, beta_dev, bias_dev, wf_out_dev, c1_out_dev, c2_out_dev, N, K, (hipStream_t)stream,
                                       dtype == MGEA_DTYPE_F16);
}

int mgea_op_attention16(const void* qkv_dev, const int32_t* mask_dev, const int32_t* cu_seqlens_dev, void* out_dev, int32_t B, int32_t T,
                        int32_t n_head, int32_t head_dim, int32_t dtype, void* pages_dev, int32_t n_pages,
                        const int32_t* page_table_dev, int32_t max_pages, void* stream) {
    MGEA_REQUIRE(qkv_dev && out_dev && n_head > 0 && (dtype == MGEA_DTYPE_BF16 || dtype == MGEA_DTYPE_F16), MGEA_EINVAL,
                 "op_attention16: NULL argument or dtype %d (bf16, f16)", dtype);
    if (!pages_dev)
        return launch_attn_bf16(qkv_dev, mask_dev, out_dev, B, T, n_head, head_dim, (hipStream_t)stream, dtype == MGEA_DTYPE_F16, nullptr,
                                cu_seqlens_dev);
    MGEA_REQUIRE(dtype == MGEA_DTYPE_F16 && !cu_seqlens_dev && page_table_dev && n_pages > 0 && max_pages > 0, MGEA_EINVAL,
                 "op_attention16: pages need fp16, a page table and padded rows");
    const KvPages pg{op_pool(pages_dev, n_pages, n_head, head_dim, 1, 0), 0, page_table_dev, max_pages};
    return launch_attn_bf16(qkv_dev, mask_dev, out_dev, B, T, n_head, head_dim, (hipStream_t)stream, 1, &pg, nullptr);
}

int mgea_op_kv_scatter_f16(const void* qkv_dev, void* pages_dev, int32_t n_pages, const int32_t* page_table_dev, int32_t max_pages,
                           const int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                           void* stream) {
    MGEA_REQUIRE(qkv_dev && pages_dev && page_table_dev && ctx_len_dev && n_pages > 0 && max_pages > 0 && B > 0 && T > 0 && n_head > 0 &&
                     head_dim > 0,
                 MGEA_EINVAL, "op_kv_scatter_f16: bad argument");
    return launch_kv_scatter_f16(qkv_dev, op_pool(pages_dev, n_pages, n_head, head_dim, 1, 0), 0, page_table_dev, max_pages, ctx_len_dev,
                                 lens_dev, B, T, n_head * head_dim, (hipStream_t)stream);
}

int mgea_op_dec_embed_f16(const int32_t* ids_dev, const int32_t* lens_dev, const int32_t* ctx_len_dev, const float* tok_emb_dev,
                          const float* pos_emb_dev, void* x_out_dev, float* rowstat_out_dev, int32_t* mask_out_dev, float eps, int32_t B,
                          int32_t T, int32_t C, int32_t vocab, int32_t pos_rows, int32_t absolute_pos, int32_t* err_flag_dev,
                          void* stream) {
    MGEA_REQUIRE(ids_dev && tok_emb_dev && pos_emb_dev && x_out_dev && rowstat_out_dev && B > 0 && T > 0 && vocab > 0 && pos_rows > 0,
                 MGEA_EINVAL, "op_dec_embed_f16: bad argument");
    return launch_dec_embed_f16(ids_dev, lens_dev, ctx_len_dev, tok_emb_dev, pos_emb_dev, x_out_dev, rowstat_out_dev, mask_out_dev, eps, B,
                                T, C, vocab, pos_rows, absolute_pos, err_flag_dev, (hipStream_t)stream);
}

int mgea_op_attention_paged(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t dtype, int32_t arith_batch,
                            const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev, const int32_t* lens_dev,
                            float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim, int32_t no_split, int32_t* info_out,
                            void* stream) {
    return mgea_op_attention_paged_ex(qkv_dev, pages_dev, n_pages, 1, 0, dtype, arith_batch, page_table_dev, max_pages, ctx_len_dev, lens_dev,
                                      out_dev, B, T, n_head, head_dim, 0, no_split, nullptr, 0, nullptr, 0, info_out, stream);
}

int mgea_op_attn_split_count(int32_t B, int32_t n_head, int32_t T, int32_t max_pages) { return attn_split_count(B, n_head, T, max_pages); }

int mgea_op_attn_split_scratch(int32_t head_dim, int64_t* part_floats_out, int64_t* count_ints_out) {
    MGEA_REQUIRE(head_dim > 0 && part_floats_out && count_ints_out, MGEA_EINVAL, "op_attn_split_scratch: bad argument");
    *part_floats_out = (int64_t)MGEA_ATTN_SPLIT_ITEMS * MGEA_ATTN_MAX_SPLIT * attn_part_floats(head_dim);
    *count_ints_out = MGEA_ATTN_SPLIT_ITEMS;
    return MGEA_OK;
}

// mgea_op_attention_paged_ex and _causal: one body, the launcher's causal flag apart
static int op_attention_paged(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t n_layer, int32_t layer, int32_t dtype,
                              int32_t arith_batch, const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev,
                              const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                              int32_t tiled_out, int32_t no_split, float* split_part_dev, int64_t split_part_floats,
                              int32_t* split_count_dev, int64_t split_count_ints, int32_t* info_out, void* stream, int causal) {
    MGEA_REQUIRE(qkv_dev && pages_dev && page_table_dev && ctx_len_dev && out_dev && B > 0 && T > 0 && n_head > 0 && n_pages > 0 &&
                     max_pages > 0 && (dtype == MGEA_DTYPE_F32 || dtype == MGEA_DTYPE_F16),
                 MGEA_EINVAL, "op_attention_paged: bad argument");
    MGEA_REQUIRE(n_layer > 0 && layer >= 0 && layer < n_layer, MGEA_EINVAL, "op_attention_paged: layer %d of %d", layer, n_layer);
    MGEA_REQUIRE(arith_batch == 0 || (arith_batch >= B && (int64_t)max_pages * arith_batch <= n_pages), MGEA_EINVAL,
                 "op_attention_paged: arith_batch %d must be >= B with max_pages * arith_batch <= n_pages", arith_batch);
    MGEA_REQUIRE(!tiled_out || ((int64_t)B * T <= MGEA_FUSED_MAX_ROWS && ((n_head * head_dim) % 32 == 0 || (int64_t)B * T <= 64)), MGEA_EINVAL,
                 "op_attention_paged: a k-tiled out holds at most %d rows (64 when its width is no multiple of 32)", MGEA_FUSED_MAX_ROWS);
    // n_layer layers of n_pages pages each, the stride the decoder sets (decoder.hip: n_pages * 2 * n_head * page elements)
    const KvPool pool = op_pool(pages_dev, n_pages, n_head, head_dim, dtype == MGEA_DTYPE_F16, arith_batch);
    hipStream_t st = (hipStream_t)stream;
    AttnSplit sp{nullptr, nullptr, MGEA_ATTN_MAX_SPLIT, MGEA_ATTN_SPLIT_ITEMS};
    DevGroup tmp;   // frees the scratch on return: the stream is synchronised first
    const size_t part_floats = (size_t)sp.max_items * sp.max_split * attn_part_floats(head_dim);
    if (!no_split && (split_part_dev || split_count_dev)) {   // the caller's scratch: neither allocated nor zeroed here (mgea.h)
        MGEA_REQUIRE(split_part_dev && split_count_dev && split_part_floats >= (int64_t)part_floats && split_count_ints >= sp.max_items, MGEA_EINVAL,
                     "op_attention_paged: the split scratch needs %lld floats and %d counters", (long long)part_floats, sp.max_items);
        sp.part = split_part_dev;
        sp.count = split_count_dev;
    } else if (!no_split) {
        MGEA_REQUIRE(tmp.alloc(&sp.part, part_floats * sizeof(float)) == MGEA_OK, MGEA_ENOMEM, "op_attention_paged: allocation of the split partials failed");
        MGEA_REQUIRE(tmp.alloc(&sp.count, (size_t)sp.max_items * sizeof(int32_t)) == MGEA_OK, MGEA_ENOMEM,
                     "op_attention_paged: allocation of the split counters failed");
        MGEA_CHECK_HIP(hipMemsetAsync(sp.count, 0, (size_t)sp.max_items * sizeof(int32_t), st));
    }
    // what the launcher will decide from the same arguments (attn_paged.hip): workgroups per (row, head, query)
    if (info_out) info_out[0] = no_split ? 1 : attn_split_count(B, n_head, T, max_pages);
    const int rc = launch_attn_paged(qkv_dev, pool, layer, page_table_dev, max_pages, ctx_len_dev, lens_dev, out_dev, B, T, n_head * head_dim,
                                     tiled_out != 0, st, no_split ? nullptr : &sp, causal);
    const hipError_t e = hipStreamSynchronize(st);
    MGEA_TRY(rc);
    MGEA_CHECK_HIP(e);
    return MGEA_OK;
}

int mgea_op_attention_paged_ex(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t n_layer, int32_t layer, int32_t dtype,
                               int32_t arith_batch, const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev,
                               const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                               int32_t tiled_out, int32_t no_split, float* split_part_dev, int64_t split_part_floats,
                               int32_t* split_count_dev, int64_t split_count_ints, int32_t* info_out, void* stream) {
    return op_attention_paged(qkv_dev, pages_dev, n_pages, n_layer, layer, dtype, arith_batch, page_table_dev, max_pages, ctx_len_dev, lens_dev,
                              out_dev, B, T, n_head, head_dim, tiled_out, no_split, split_part_dev, split_part_floats, split_count_dev,
                              split_count_ints, info_out, stream, 0);
}

int mgea_op_attention_paged_causal(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t n_layer, int32_t layer, int32_t dtype,
                                   int32_t arith_batch, const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev,
                                   const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                                   int32_t tiled_out, int32_t no_split, float* split_part_dev, int64_t split_part_floats,
                                   int32_t* split_count_dev, int64_t split_count_ints, int32_t* info_out, void* stream) {
    return op_attention_paged(qkv_dev, pages_dev, n_pages, n_layer, layer, dtype, arith_batch, page_table_dev, max_pages, ctx_len_dev, lens_dev,
                              out_dev, B, T, n_head, head_dim, tiled_out, no_split, split_part_dev, split_part_floats, split_count_dev,
                              split_count_ints, info_out, stream, 1);
}

/* ablation / micro-benchmark hook for the fused skinny GEMM (tools/skinny_bench.py): EPI_ACT or
 * EPI_RES on caller buffers; dbg bits skip A loads (1), W loads (2), MFMAs (4). */
int64_t mgea_op_tiled_weight_floats(int32_t N, int32_t K) { return wtile_floats(N, K); }

int mgea_op_tile_weights(const float* w_dev, int32_t N, int32_t K, float* out_dev, void* stream) {
    return launch_tile_weights(w_dev, N, K, out_dev, (hipStream_t)stream);
}

int mgea_op_fold_ln(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                    float* wt_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream) {
    return launch_ln_fold(w_dev, gamma_dev, beta_dev, bias_dev, N, K, wt_out_dev, c1_out_dev, c2_out_dev, (hipStream_t)stream);
}

int mgea_op_tile_rows(const float* src_dev, float* dst_dev, int32_t M, int32_t N, int32_t to_tiled, void* stream) {
    return launch_tile_rows(src_dev, dst_dev, M, N, to_tiled, (hipStream_t)stream);
}

int mgea_op_skinny(int32_t epi, const float* a_dev, const float* w_dev, const float* bias_dev, const float* ln_c1_dev,
                   const float* stats_in_dev, int32_t n_part, int32_t part_cnt, float* out_dev,
                   float* stats_out_dev, int32_t M, int32_t N, int32_t K, int32_t act, int32_t dbg, void* stream) {
    SkinnyArgs a{};
    a.A = a_dev; a.lda = K; a.W = w_dev; a.bias = bias_dev; a.M = M; a.N = N; a.K = K;
    a.ln_c1 = ln_c1_dev; a.eps = 1e-5f; a.stats_in = stats_in_dev; a.n_part = n_part; a.part_cnt = part_cnt;
    a.out = out_dev; a.ldo = N; a.stats_out = stats_out_dev; a.act = act; a.dbg = dbg;
    MGEA_REQUIRE(epi == EPI_ACT || epi == EPI_RES || epi == EPI_LOGITS, MGEA_EINVAL, "op_skinny: epilogue %d not exposed", epi);
    MGEA_REQUIRE(epi != EPI_LOGITS || stats_out_dev, MGEA_EINVAL, "op_skinny: the LOGITS epilogue writes its partials to stats_out_dev");
    DecodeGemmPlan p;
    MGEA_TRY(plan_decode_gemm(epi, a, false, &p));
    if (epi == EPI_LOGITS) {   // LM head: logits [M,N] row-major in out_dev (or NULL); (max, argmax) partials in stats_out_dev (mgea.h)
        a.pmax_val = stats_out_dev;
        a.pmax_idx = reinterpret_cast<int32_t*>(stats_out_dev + (int64_t)(M > 64 ? M : 64) * p.n_partials);
    }
    return launch_decode_gemm(epi, p, a, (hipStream_t)stream);
}

int mgea_op_skinny_logits_partials(int32_t M, int32_t N, int32_t K) {
    SkinnyArgs a{};
    a.M = M; a.N = N; a.K = K;   // (no LayerNorm, dbg = 0)
    DecodeGemmPlan p;
    return plan_decode_gemm(EPI_LOGITS, a, false, &p) == MGEA_OK ? p.n_partials : 0;
}

// test-only: any decode-GEMM plan on caller buffers (mgea.h).  Fills the argument block, plans, launches that plan, synchronises.
int mgea_op_decode_gemm(const mgea_decode_gemm_args* g, int32_t* plan_out, void* stream) {
    for (int i = 0; plan_out && i < MGEA_DECODE_GEMM_PLAN_INTS; ++i) plan_out[i] = -1;
    MGEA_REQUIRE(g && g->a_dev && g->w_dev && g->M > 0 && g->N > 0 && g->K > 0, MGEA_EINVAL, "op_decode_gemm: bad argument");
    MGEA_REQUIRE(g->epi == EPI_QKV ? g->arith_batch >= 0 : g->arith_batch == 0, MGEA_EINVAL, "op_decode_gemm: arith_batch %d (QKV only, >= 0)", g->arith_batch);
    const int epi = g->epi;
    MGEA_REQUIRE(epi >= EPI_QKV && epi <= EPI_LOGITS, MGEA_EINVAL, "op_decode_gemm: bad epilogue %d", epi);
    MGEA_REQUIRE(epi == EPI_LOGITS ? g->partials_dev != nullptr : g->out_dev != nullptr, MGEA_EINVAL,
                 "op_decode_gemm: the epilogue's output buffer is NULL");
    MGEA_REQUIRE(!g->ln_c1_dev || (g->stats_in_dev && g->n_part > 0 && g->part_cnt > 0), MGEA_EINVAL,
                 "op_decode_gemm: the folded LayerNorm needs stats_in_dev, n_part and part_cnt");
    SkinnyArgs a{};
    a.A = g->a_dev; a.lda = g->K; a.W = static_cast<const float*>(g->w_dev); a.w_f16 = g->w_f16 != 0; a.bias = g->bias_dev;
    a.M = g->M; a.N = g->N; a.K = g->K;
    a.ln_c1 = g->ln_c1_dev; a.eps = g->eps; a.ln_g = g->ln_g_dev; a.ln_b = g->ln_b_dev;
    a.stats_in = g->stats_in_dev; a.n_part = g->n_part; a.part_cnt = g->part_cnt;
    a.out = g->out_dev; a.ldo = g->N; a.stats_out = g->stats_out_dev; a.act = g->act;
    if (epi == EPI_QKV) {
        MGEA_REQUIRE(g->pages_dev && g->page_table_dev && g->ctx_len_dev && g->n_pages > 0 && g->max_pages > 0 && g->n_head > 0 &&
                         g->head_dim > 0 && g->head_dim % 8 == 0 && g->layer >= 0 && g->T >= 1 && g->M % g->T == 0 &&
                         g->N == 3 * g->n_head * g->head_dim && (g->page_dtype == MGEA_DTYPE_F32 || g->page_dtype == MGEA_DTYPE_F16),
                     MGEA_EINVAL, "op_decode_gemm: bad QKV argument (N = 3 * n_head * head_dim, M a multiple of T, fp32 or fp16 pages)");
        MGEA_REQUIRE(g->arith_batch == 0 || (g->arith_batch >= g->M / g->T && (int64_t)g->max_pages * g->arith_batch <= g->n_pages), MGEA_EINVAL,
                     "op_decode_gemm: arith_batch %d must be >= M / T with max_pages * arith_batch <= n_pages", g->arith_batch);
        a.pool = op_pool(g->pages_dev, g->n_pages, g->n_head, g->head_dim, g->page_dtype == MGEA_DTYPE_F16, g->arith_batch);
        a.layer = g->layer; a.page_table = g->page_table_dev; a.max_pages = g->max_pages; a.ctx_len = g->ctx_len_dev;
        a.lens = g->lens_dev; a.T = g->T; a.C = g->n_head * g->head_dim;
    }
    DecodeGemmPlan p;
    MGEA_TRY(plan_decode_gemm(epi, a, g->rowmajor != 0, &p));
    if (epi == EPI_LOGITS) {   // the partials layout of mgea_op_skinny_logits_partials
        a.pmax_val = g->partials_dev;
        a.pmax_idx = reinterpret_cast<int32_t*>(g->partials_dev + (int64_t)(g->M > 64 ? g->M : 64) * p.n_partials);
    }
    if (plan_out) {
        const int v[MGEA_DECODE_GEMM_PLAN_INTS] = {p.kind, p.mt, p.nt, p.nw, p.nch, p.cw, p.mr, p.base, (int)p.grid.x, (int)p.grid.y,
                                                   p.n_partials};
        for (int i = 0; i < MGEA_DECODE_GEMM_PLAN_INTS; ++i) plan_out[i] = v[i];
    }
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_decode_gemm(epi, p, a, st);
    const hipError_t e = hipStreamSynchronize(st);
    MGEA_TRY(rc);
    MGEA_CHECK_HIP(e);
    return MGEA_OK;
}

int mgea_op_tile_weights_f16(const float* w_dev, int32_t N, int32_t K, void* out_dev, void* stream) {
    return launch_tile_weights_f16(w_dev, N, K, out_dev, (hipStream_t)stream);
}

int mgea_op_ln_vectors(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                       float* c1_out_dev, float* c2_out_dev, void* stream) {
    MGEA_REQUIRE(N > 0 && K > 0, MGEA_EINVAL, "op_ln_vectors: N=%d K=%d", N, K);
    return launch_ln_vectors(w_dev, gamma_dev, beta_dev, bias_dev, N, K, c1_out_dev, c2_out_dev, (hipStream_t)stream);
}

int mgea_op_sample(const float* logits_dev, int32_t B, int32_t V, const mgea_sampler_config* s, int64_t step,
                   int32_t* ids_out_dev, float* probs_out_dev, void* stream) {
    MGEA_REQUIRE(logits_dev && s, MGEA_EINVAL, "op_sample: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    SampleCall c = op_sample_call(logits_dev, B, V, step, ids_out_dev, probs_out_dev);
    c.params = sampler_params(*s);
    if (s->top_k == 1 && ids_out_dev) {
        MGEA_TRY(launch_logits_argmax(logits_dev, 1, 0, V, nullptr, nullptr, B, V, ids_out_dev, st));
        if (!probs_out_dev) return MGEA_OK;
        c.ids_out = nullptr;
    }
    return launch_sample(c, st);
}

int mgea_op_sample_penalized(const float* logits_dev, int32_t B, int32_t V, const mgea_sampler_config* s, float repetition_penalty,
                             const uint32_t* presence_dev, int64_t step, int32_t* ids_out_dev, float* probs_out_dev, void* stream) {
    MGEA_REQUIRE(logits_dev && s, MGEA_EINVAL, "op_sample_penalized: NULL argument");
    MGEA_REQUIRE(std::isfinite(repetition_penalty) && repetition_penalty > 0.f, MGEA_EINVAL,
                 "op_sample_penalized: repetition_penalty must be finite and > 0 (got %g)", (double)repetition_penalty);
    if (repetition_penalty == 1.0f) return mgea_op_sample(logits_dev, B, V, s, step, ids_out_dev, probs_out_dev, stream);
    MGEA_REQUIRE(presence_dev, MGEA_EINVAL, "op_sample_penalized: presence_dev is NULL");
    SampleCall c = op_sample_call(logits_dev, B, V, step, ids_out_dev, probs_out_dev);
    c.params = sampler_params(*s, repetition_penalty);
    c.presence = const_cast<uint32_t*>(presence_dev);   // the kernel only reads the bitmap (it writes one only in the decoder's fused tail)
    return launch_sample(c, (hipStream_t)stream);
}

int mgea_op_sample_rows(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                        int64_t step, int32_t* ids_out_dev, float* probs_out_dev, void* stream) {
    return mgea_op_sample_rows_biased(logits_dev, B, V, rows, presence_dev, nullptr, step, ids_out_dev, probs_out_dev, stream);
}

int mgea_op_sample_rows_biased(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows,
                               const uint32_t* presence_dev, const mgea_row_logits* lrows, int64_t step, int32_t* ids_out_dev,
                               float* probs_out_dev, void* stream) {
    return op_sample_rows(logits_dev, B, V, rows, presence_dev, lrows, step, ids_out_dev, probs_out_dev, ScoreArgs{}, stream);
}

int mgea_op_sample_rows_scored(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows,
                               const uint32_t* presence_dev, const mgea_row_logits* lrows, int64_t step, int32_t* ids_out_dev,
                               float* probs_out_dev, const int32_t* forced_ids_dev, float* logprobs_out_dev,
                               float* choice_logprobs_out_dev, void* stream) {
    MGEA_REQUIRE(ids_out_dev && logprobs_out_dev, MGEA_EINVAL, "op_sample_rows_scored: ids_out_dev or logprobs_out_dev is NULL");
    // forced [B] (stride 0), the values to [B] vectors, no error flag here: a forced id >= V is clamped silently
    return op_sample_rows(logits_dev, B, V, rows, presence_dev, lrows, step, ids_out_dev, probs_out_dev,
                          ScoreArgs{forced_ids_dev, 0, logprobs_out_dev, choice_logprobs_out_dev, 0, nullptr}, stream);
}

int mgea_op_window_evict(int32_t* page_table_dev, int32_t max_pages, int32_t sink_pages, int32_t ring_pages, int32_t* ctx_len_dev,
                         const int32_t* done_dev, int32_t* evictions_dev, int32_t B, void* stream) {
    return launch_window_evict(page_table_dev, max_pages, sink_pages, ring_pages, ctx_len_dev, done_dev, evictions_dev, B,
                               (hipStream_t)stream);
}

int mgea_op_guidance_mix(float* logits_dev, int32_t B, int32_t V, const int32_t* partner_dev, const float* scale_dev, void* stream) {
    return launch_guidance_mix(logits_dev, B, V, partner_dev, scale_dev, (hipStream_t)stream);
}

int mgea_op_blend_mix(float* logits_dev, int32_t B, int32_t V, const int32_t* leader_dev, const float* weight_dev, void* stream) {
    return launch_blend_mix(logits_dev, B, V, leader_dev, weight_dev, (hipStream_t)stream);
}

int mgea_op_class_penalty(float* logits_dev, int32_t B, int32_t V, const int32_t* class_of_dev, int32_t n_class, const int32_t* hist_dev,
                          int32_t stride, const int32_t* row_step_dev, const int32_t* done_dev, const mgea_row_class_penalty* recs_host,
                          void* stream) {
    MGEA_REQUIRE(logits_dev && class_of_dev && hist_dev && row_step_dev && done_dev && recs_host && B > 0, MGEA_EINVAL,
                 "op_class_penalty: NULL argument or empty batch");
    MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "op_class_penalty: vocab %d exceeds the sampler's row (%d)", V,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(n_class >= 1 && n_class <= V, MGEA_EINVAL, "op_class_penalty: n_class %d outside [1, %d]", n_class, V);
    MGEA_REQUIRE(stride > 0, MGEA_EINVAL, "op_class_penalty: history stride %d must be > 0", stride);
    int n_on = 0;
    MGEA_TRY(check_row_class_penalty(recs_host, B, -1, n_class, "op_class_penalty", &n_on));
    hipStream_t st = (hipStream_t)stream;
    mgea_row_class_penalty* recs_dev = nullptr;
    DevGroup g;   // nothing is enqueued before the allocation, and the stream is synchronised before it is freed
    MGEA_REQUIRE(g.alloc(&recs_dev, (size_t)B * sizeof(mgea_row_class_penalty)) == MGEA_OK, MGEA_ENOMEM,
                 "op_class_penalty: allocation of the records failed");
    int rc = MGEA_EHIP;
    if (hipMemcpyAsync(recs_dev, recs_host, (size_t)B * sizeof(mgea_row_class_penalty), hipMemcpyHostToDevice, st) == hipSuccess)
        rc = launch_class_penalty(logits_dev, B, V, class_of_dev, n_class, hist_dev, stride, row_step_dev, done_dev, recs_dev, st);
    else
        set_error("op_class_penalty: copy of the records failed");
    const hipError_t e = hipStreamSynchronize(st);
    MGEA_TRY(rc);
    MGEA_CHECK_HIP(e);
    return MGEA_OK;
}

int mgea_op_recondition(void* pool_dev, int32_t n_layer, int32_t n_pages, int32_t H, int32_t dh, int32_t f16, int32_t arith_batch,
                        const int32_t* page_table_dev, int32_t max_pages, void* store_dev, int32_t n_seg_max, int32_t slot_tokens,
                        int32_t* meta_dev, int32_t* len_dev, int32_t B, int32_t gather_seg, const int32_t* lens_dev,
                        const mgea_row_schedule* sched_dev, const int32_t* done_dev, const int32_t* row_step_dev,
                        const int32_t* gram_state_dev, int32_t* cur_seg_dev, int32_t* switches_dev, void* stream) {
    MGEA_REQUIRE(n_seg_max >= 1 && n_seg_max <= MGEA_SCHEDULE_MAX_SEGMENTS, MGEA_EINVAL, "op_recondition: n_seg_max %d outside [1, %d]", n_seg_max,
                 MGEA_SCHEDULE_MAX_SEGMENTS);
    MGEA_REQUIRE(slot_tokens >= 1 && slot_tokens <= MGEA_KV_PAGE_TOKENS, MGEA_EINVAL, "op_recondition: slot_tokens %d outside [1, %d]", slot_tokens,
                 MGEA_KV_PAGE_TOKENS);
    MGEA_REQUIRE(gather_seg < n_seg_max, MGEA_EINVAL, "op_recondition: gather_seg %d of %d segments", gather_seg, n_seg_max);
    MGEA_REQUIRE(gather_seg >= 0 || sched_dev, MGEA_EINVAL, "op_recondition: neither a gather nor an apply");
    MGEA_REQUIRE(!sched_dev || (done_dev && row_step_dev && gram_state_dev && cur_seg_dev && switches_dev), MGEA_EINVAL,
                 "op_recondition: an apply needs done, row_step, gram_state, cur_seg and switches");
    KvPool pool{};
    pool.base = pool_dev; pool.n_pages = n_pages; pool.H = H; pool.dh = dh; pool.f16 = f16; pool.arith_batch = arith_batch;
    pool.layer_stride = (int64_t)n_pages * 2 * H * pool.page_elems();
    if (gather_seg >= 0)
        MGEA_TRY(launch_cond_gather(pool, n_layer, page_table_dev, max_pages, lens_dev, slot_tokens, store_dev, gather_seg, n_seg_max, slot_tokens,
                                    meta_dev, len_dev, B, (hipStream_t)stream));
    if (sched_dev)
        MGEA_TRY(launch_cond_apply(pool, n_layer, page_table_dev, max_pages, store_dev, meta_dev, len_dev, sched_dev, done_dev, row_step_dev,
                                   gram_state_dev, cur_seg_dev, switches_dev, B, (hipStream_t)stream));
    return MGEA_OK;
}

int mgea_op_sample_rows_grammar(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                                const mgea_row_logits* lrows, const int32_t* class_of_dev, const int32_t* next_dev, int32_t n_state,
                                int32_t n_class, const int32_t* states_in_dev, int64_t step, int32_t* ids_out_dev, float* probs_out_dev,
                                int32_t* states_out_dev, void* stream) {
    MGEA_REQUIRE(class_of_dev && next_dev && states_in_dev && (states_out_dev || !ids_out_dev), MGEA_EINVAL,
                 "op_sample_rows_grammar: NULL table or state argument");
    MGEA_REQUIRE(n_class >= 1 && n_class <= MGEA_GRAMMAR_MAX_CLASSES && n_state >= 1 && n_state <= MGEA_GRAMMAR_MAX_STATES &&
                     (int64_t)n_state * n_class <= MGEA_GRAMMAR_MAX_CELLS,
                 MGEA_EINVAL, "op_sample_rows_grammar: n_state %d x n_class %d exceed the caps", n_state, n_class);
    // states_out starts as states_in: rows the sampler does not move (state -1) keep theirs
    if (states_out_dev)
        MGEA_CHECK_HIP(hipMemcpyAsync(states_out_dev, states_in_dev, (size_t)(B > 0 ? B : 0) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream));
    const GrammarArgs g{class_of_dev, next_dev, nullptr, states_in_dev, states_out_dev, nullptr, n_state, n_class, 0, nullptr};
    return op_sample_rows(logits_dev, B, V, rows, presence_dev, lrows, step, ids_out_dev, probs_out_dev, ScoreArgs{}, stream, &g);
}

int mgea_op_sample_rows_truncated(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                                  const mgea_row_logits* lrows, const mgea_row_truncation* trunc, int64_t step, int32_t* ids_out_dev,
                                  float* probs_out_dev, const int32_t* forced_ids_dev, float* logprobs_out_dev,
                                  float* choice_logprobs_out_dev, const int32_t* class_of_dev, const int32_t* next_dev, int32_t n_state,
                                  int32_t n_class, const int32_t* states_in_dev, int32_t* states_out_dev, void* stream) {
    MGEA_REQUIRE(logprobs_out_dev || (!forced_ids_dev && !choice_logprobs_out_dev), MGEA_EINVAL,
                 "op_sample_rows_truncated: forced ids and choice log-probabilities need logprobs_out_dev");
    MGEA_REQUIRE(!logprobs_out_dev || ids_out_dev, MGEA_EINVAL, "op_sample_rows_truncated: a scored launch needs ids_out_dev");
    const ScoreArgs score = logprobs_out_dev ? ScoreArgs{forced_ids_dev, 0, logprobs_out_dev, choice_logprobs_out_dev, 0, nullptr} : ScoreArgs{};
    if (!class_of_dev) return op_sample_rows(logits_dev, B, V, rows, presence_dev, lrows, step, ids_out_dev, probs_out_dev, score, stream, nullptr, trunc);
    MGEA_REQUIRE(next_dev && states_in_dev && (states_out_dev || !ids_out_dev), MGEA_EINVAL,
                 "op_sample_rows_truncated: NULL table or state argument");
    MGEA_REQUIRE(n_class >= 1 && n_class <= MGEA_GRAMMAR_MAX_CLASSES && n_state >= 1 && n_state <= MGEA_GRAMMAR_MAX_STATES &&
                     (int64_t)n_state * n_class <= MGEA_GRAMMAR_MAX_CELLS,
                 MGEA_EINVAL, "op_sample_rows_truncated: n_state %d x n_class %d exceed the caps", n_state, n_class);
    if (states_out_dev)   // rows the sampler does not move keep their state (mgea_op_sample_rows_grammar)
        MGEA_CHECK_HIP(hipMemcpyAsync(states_out_dev, states_in_dev, (size_t)(B > 0 ? B : 0) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream));
    const GrammarArgs g{class_of_dev, next_dev, nullptr, states_in_dev, states_out_dev, nullptr, n_state, n_class, 0, nullptr};
    return op_sample_rows(logits_dev, B, V, rows, presence_dev, lrows, step, ids_out_dev, probs_out_dev, score, stream, &g, trunc);
}

// ---- the DistilBERT row, [CLS] and split-K epilogue kernels, one launch per call (tests) ----
int mgea_op_attention_cls(const float* q_dev, const void* qkv_dev, int32_t kv_dtype, const int32_t* mask_dev,
                          const int32_t* cu_seqlens_dev, float* out_dev, int32_t B, int32_t S, int32_t n_head, int32_t head_dim,
                          void* stream) {
    MGEA_REQUIRE(q_dev && qkv_dev && out_dev && B > 0 && n_head > 0 && (cu_seqlens_dev || S > 0), MGEA_EINVAL, "op_attention_cls: bad argument");
    MGEA_REQUIRE(kv_dtype == MGEA_DTYPE_F32 || kv_dtype == MGEA_DTYPE_BF16, MGEA_EINVAL, "op_attention_cls: K | V dtype %d (f32, bf16)", kv_dtype);
    return launch_attn_cls(q_dev, qkv_dev, kv_dtype == MGEA_DTYPE_BF16, mask_dev, out_dev, B, S, n_head, head_dim, (hipStream_t)stream,
                           cu_seqlens_dev);
}

int mgea_op_bert_embed(const int32_t* ids_dev, const int32_t* pos_ids_dev, const float* word_dev, const float* pos_dev,
                       const float* ln_w_dev, const float* ln_b_dev, float eps, void* out_dev, int32_t out_dtype, int32_t B, int32_t S,
                       int32_t D, int32_t vocab, int32_t* err_flag_dev, void* stream) {
    MGEA_REQUIRE(ids_dev && word_dev && pos_dev && ln_w_dev && ln_b_dev && out_dev && B > 0 && S > 0 && D > 0 && vocab > 0, MGEA_EINVAL,
                 "op_bert_embed: bad argument");
    MGEA_REQUIRE(out_dtype == MGEA_DTYPE_F32 || out_dtype == MGEA_DTYPE_BF16, MGEA_EINVAL, "op_bert_embed: output dtype %d (f32, bf16)", out_dtype);
    if (out_dtype == MGEA_DTYPE_BF16)
        return launch_bert_embed_ln_bf16(ids_dev, word_dev, pos_dev, ln_w_dev, ln_b_dev, eps, out_dev, B, S, D, vocab, (hipStream_t)stream,
                                         err_flag_dev, pos_ids_dev);
    return launch_bert_embed_ln(ids_dev, word_dev, pos_dev, ln_w_dev, ln_b_dev, eps, static_cast<float*>(out_dev), B, S, D, vocab,
                                (hipStream_t)stream, err_flag_dev, pos_ids_dev);
}

int mgea_op_gather_cls(const void* h_dev, int32_t dtype, const float* rowstat_dev, const float* ln_g_dev, const float* ln_b_dev,
                       const int32_t* cu_dev, float* out_dev, int32_t B, int32_t S, int32_t D, void* stream) {
    MGEA_REQUIRE(h_dev && out_dev && B > 0 && D > 0 && (cu_dev || S > 0), MGEA_EINVAL, "op_gather_cls: bad argument");
    MGEA_REQUIRE(dtype == MGEA_DTYPE_F32 || dtype == MGEA_DTYPE_BF16, MGEA_EINVAL, "op_gather_cls: dtype %d (f32, bf16)", dtype);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MGEA_DTYPE_F32) {
        MGEA_REQUIRE(!rowstat_dev && D % 4 == 0, MGEA_EINVAL, "op_gather_cls: fp32 rows are copied (no rowstat, D %% 4 == 0)");
        return launch_gather_rows(static_cast<const float*>(h_dev), D, out_dev, D, B, S, D, st, cu_dev);
    }
    if (!rowstat_dev) return launch_gather_cls_bf16(h_dev, out_dev, B, S, D, st, cu_dev);
    MGEA_REQUIRE(ln_g_dev && ln_b_dev, MGEA_EINVAL, "op_gather_cls: the LayerNorm form needs ln_g_dev and ln_b_dev");
    return launch_gather_cls_ln_bf16(h_dev, rowstat_dev, ln_g_dev, ln_b_dev, out_dev, B, S, D, st, cu_dev);
}

int mgea_op_gemm_f32_direct(const float* a_dev, int32_t lda, const float* w_dev, int32_t ldw, const float* bias_dev, float* out_dev,
                            int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t act, void* stream) {
    MGEA_REQUIRE(a_dev && w_dev && out_dev && N > 0 && K > 0 && lda >= K && ldw >= K && lda % 4 == 0 && ldw % 4 == 0, MGEA_EINVAL,
                 "op_gemm_f32_direct: bad argument (lda, ldw >= K and multiples of 4)");
    MGEA_REQUIRE(act == ACT_NONE || act == ACT_GELU || act == ACT_RELU, MGEA_EINVAL, "op_gemm_f32_direct: act %d", act);
    return launch_gemm_f32_bias_act(a_dev, lda, w_dev, ldw, bias_dev, out_dev, ldo, M, N, K, act, (hipStream_t)stream);
}

// the slab geometry every epilogue kernel relies on: 16-byte loads of whole groups of `row` columns
static int check_slabs(const char* who, const float* p_dev, int32_t S, int64_t ps, int32_t ldp, int32_t M, int32_t row) {
    MGEA_REQUIRE(p_dev && S >= 1 && M > 0 && row > 0 && ldp % 4 == 0 && ldp >= round_up(row, 4) && (S == 1 || (ps % 4 == 0 && ps >= (int64_t)M * ldp)),
                 MGEA_EINVAL, "%s: bad slabs (S=%d ps=%lld ldp=%d for %d rows of %d columns)", who, S, (long long)ps, ldp, M, row);
    return MGEA_OK;
}

int mgea_op_slab_bias_act(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* out_dev, int32_t ldo,
                          int32_t M, int32_t N, int32_t act, void* stream) {
    MGEA_TRY(check_slabs("op_slab_bias_act", p_dev, S, ps, ldp, M, N));
    MGEA_REQUIRE(out_dev && ldo >= N && (act == ACT_NONE || act == ACT_GELU || act == ACT_RELU), MGEA_EINVAL,
                 "op_slab_bias_act: bad argument (ldo=%d N=%d act=%d)", ldo, N, act);
    return launch_bias_act(p_dev, S, ps, ldp, bias_dev, out_dev, ldo, M, N, act, (hipStream_t)stream);
}

int mgea_op_slab_bias_res_ln(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* x_dev, float* xn_dev,
                             const float* ln_w_dev, const float* ln_b_dev, float eps, int32_t M, int32_t C, int32_t post_ln,
                             void* stream) {
    MGEA_TRY(check_slabs("op_slab_bias_res_ln", p_dev, S, ps, ldp, M, C));
    MGEA_REQUIRE(x_dev && (!ln_w_dev || (ln_b_dev && (post_ln || xn_dev))), MGEA_EINVAL,
                 "op_slab_bias_res_ln: x_dev is NULL, or LayerNorm weights without ln_b_dev / xn_dev");
    return launch_bias_res_ln(p_dev, S, ps, ldp, bias_dev, x_dev, xn_dev, ln_w_dev, ln_b_dev, eps, M, C, post_ln, (hipStream_t)stream);
}

int mgea_op_slab_logits_argmax(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* logits_dev,
                               int32_t M, int32_t V, int32_t* argmax_dev, void* stream) {
    MGEA_REQUIRE(p_dev && S >= 1 && M > 0 && V > 0 && ldp >= V && (S == 1 || ps >= (int64_t)M * ldp), MGEA_EINVAL,
                 "op_slab_logits_argmax: bad slabs (S=%d ps=%lld ldp=%d for %d rows of %d columns)", S, (long long)ps, ldp, M, V);
    return launch_logits_argmax(p_dev, S, ps, ldp, bias_dev, logits_dev, M, V, argmax_dev, (hipStream_t)stream);
}

int mgea_op_slab_qkv_scatter(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* qkv_out_dev,
                             void* pages_dev, int32_t n_pages, int32_t page_dtype, const int32_t* page_table_dev, int32_t max_pages,
                             const int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t n_head,
                             int32_t head_dim, void* stream) {
    MGEA_REQUIRE(pages_dev && page_table_dev && ctx_len_dev && n_pages > 0 && max_pages > 0 && B > 0 && T > 0 && n_head > 0 && head_dim > 0 &&
                     head_dim % 8 == 0 && (page_dtype == MGEA_DTYPE_F32 || page_dtype == MGEA_DTYPE_F16),
                 MGEA_EINVAL, "op_slab_qkv_scatter: bad argument (head_dim %% 8 == 0, fp32 or fp16 pages)");
    const int C = n_head * head_dim;
    MGEA_TRY(check_slabs("op_slab_qkv_scatter", p_dev, qkv_out_dev ? S : 1, ps, ldp, B * T, 3 * C));
    return launch_qkv_scatter(p_dev, S, ps, ldp, bias_dev, qkv_out_dev, op_pool(pages_dev, n_pages, n_head, head_dim, page_dtype == MGEA_DTYPE_F16, 0),
                              0, page_table_dev, max_pages, ctx_len_dev, lens_dev, B, T, C, (hipStream_t)stream);
}

// ---- the kernels that end a decode step and the decoder's prefill row kernels, one launch per call (tests) ----
// the launch's status and the stream's, in that order
static int op_finish(int rc, hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    MGEA_TRY(rc);
    MGEA_CHECK_HIP(e);
    return MGEA_OK;
}

int mgea_op_step_tail(const mgea_step_tail_args* a, void* stream) {
    MGEA_REQUIRE(a && !a->reserved && !a->reserved2 && a->kind >= 0 && a->kind <= 4, MGEA_EINVAL, "op_step_tail: NULL block, reserved != 0 or bad kind");
    const int kind = a->kind, B = a->B;
    MGEA_REQUIRE(B >= 1 && B <= MGEA_FUSED_MAX_ROWS, MGEA_EINVAL, "op_step_tail: %d rows (1..%d)", B, MGEA_FUSED_MAX_ROWS);
    MGEA_REQUIRE(a->cur_ids_dev && a->ctx_len_dev && (kind == 3 || (a->done_dev && a->row_step_dev && a->n_done_dev && a->sampled_dev)) &&
                     a->n_steps >= 0,
                 MGEA_EINVAL, "op_step_tail: the rows' state is incomplete");
    hipStream_t st = (hipStream_t)stream;
    const bool embeds = kind == 1 || kind == 3 || kind == 4, table = a->qkv0_dev != nullptr;
    TailArgs t{};
    t.s = StepState{a->cur_ids_dev, a->ctx_len_dev, a->done_dev, a->row_step_dev, a->n_done_dev, a->ids_out_dev, a->n_steps, a->eos_id, nullptr};
    if (embeds) {
        MGEA_REQUIRE(a->tok_emb_dev && a->pos_emb_dev && a->x_dev && (table || kind == 3 || a->stats_dev) && a->C > 0 && a->vocab > 0 &&
                         a->pos_rows > 0,
                     MGEA_EINVAL, "op_step_tail: the embedding's arguments are incomplete");
        // k-tiled x: a width that is no multiple of 32 leaves its last k-chunk partly used, and the next 64-row group would start inside it
        MGEA_REQUIRE(a->C % 32 == 0 || B <= 64, MGEA_EINVAL, "op_step_tail: a k-tiled x of width %d (no multiple of 32) holds at most 64 rows", a->C);
        t.tok_emb = a->tok_emb_dev; t.pos_emb = a->pos_emb_dev; t.x = a->x_dev; t.stats = a->stats_dev;
        t.C = a->C; t.vocab = a->vocab; t.pos_rows = a->pos_rows; t.absolute_pos = a->absolute_pos;
        if (table) {
            MGEA_REQUIRE(a->n_pages > 0 && a->max_pages > 0 && a->n_head > 0 && a->head_dim > 0 && a->head_dim % 4 == 0 &&
                             (a->page_dtype == MGEA_DTYPE_F32 || a->page_dtype == MGEA_DTYPE_F16) &&
                             (a->arith_batch > 0 ? a->arith_batch >= B && (int64_t)a->max_pages * a->arith_batch <= a->n_pages
                                                 : a->arith_batch == 0 && a->page_table_dev != nullptr),
                         MGEA_EINVAL, "op_step_tail: bad page image (a page table, or arith_batch >= B with max_pages * arith_batch <= n_pages)");
            t.qkv0 = a->qkv0_dev; t.qkv = a->qkv_dev;
            t.pool = op_pool(a->pages_dev, a->n_pages, a->n_head, a->head_dim, a->page_dtype == MGEA_DTYPE_F16, a->arith_batch);
            t.page_table = a->page_table_dev; t.max_pages = a->max_pages;
        }
    }
    const bool scored = a->logprob_hist_dev != nullptr, grammar = kind == 4 && a->class_of_dev != nullptr;
    const int V = kind == 4 ? a->vocab : a->V;
    if (kind == 0 || kind == 1) MGEA_REQUIRE(a->pval_dev && a->pidx_dev && a->n_tiles >= 1, MGEA_EINVAL, "op_step_tail: no partials");
    if (kind == 2)
        MGEA_REQUIRE((!a->presence_dev || V > 0) && (!scored || (a->logprob_step_dev && a->choice_step_dev && a->choice_hist_dev && a->hist_stride >= 0)),
                     MGEA_EINVAL, "op_step_tail: advance: a bitmap without V, or an incomplete score file");
    if (kind == 4) {
        MGEA_REQUIRE(a->logits_dev && a->rows && a->V == a->vocab && (!scored || a->hist_stride >= 0) && (scored || !a->forced_dev) &&
                         a->forced_stride >= 0,
                     MGEA_EINVAL, "op_step_tail: sampler: logits, records, V == vocab; forced ids need the histories");
        MGEA_REQUIRE(!grammar || (a->next_dev && a->states_dev && a->n_class >= 1 && a->n_class <= MGEA_GRAMMAR_MAX_CLASSES && a->n_state >= 1 &&
                                  a->n_state <= MGEA_GRAMMAR_MAX_STATES && (int64_t)a->n_state * a->n_class <= MGEA_GRAMMAR_MAX_CELLS),
                     MGEA_EINVAL, "op_step_tail: sampler: bad grammar arguments");
    }
    if (kind == 4)   // launch_sample's own refusals, taken before anything is enqueued
        MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB && t.C % 4 == 0 && t.C <= 4096 && tail_qkv0_ok(t), MGEA_EINVAL,
                     "op_step_tail: sampler: vocab %d or the fused tail's shape is refused", V);
    // the rows' records, and the sampler's other temporaries -> device buffers (freed on return: the stream is synchronised first)
    std::vector<SamplerParams> rec;
    RowsStage stage;
    const mgea_row_logits* lrows = kind == 4 ? a->logits_rows : nullptr;
    // as mgea_op_sample_rows_grammar builds it: the allow bitmask by its own kernel, empty bitmaps where none came
    const GrammarArgs g{a->class_of_dev, a->next_dev, nullptr, a->states_dev, a->states_dev, a->done_dev,
                        a->n_state, a->n_class, grammar_words(a->n_class), a->err_flag_dev};
    SampleCall c{};
    c.logits = a->logits_dev; c.B = B; c.V = V; c.ids_out = a->sampled_dev; c.row_step_dev = a->row_step_dev;
    c.tail = &t;
    c.presence = a->presence_dev;
    if (a->rows) {
        MGEA_TRY(check_row_samplers(a->rows, B, kind == 4 ? V : MGEA_SAMPLER_MAX_VOCAB, -1, "op_step_tail"));
        if (lrows) MGEA_TRY(check_row_logits(lrows, B, -1, "op_step_tail"));
        rec.resize((size_t)B);
        build_row_records(a->rows, lrows, B, -1, rec.data());
        for (int b = 0; a->ctx_cap && b < B; ++b) rec[b].ctx_cap = a->ctx_cap[b];
        const int bad = stage.alloc(B, V, true, lrows || grammar, grammar ? &g : nullptr, false, a->presence_dev != nullptr);
        MGEA_REQUIRE(!bad, MGEA_ENOMEM, "op_step_tail: allocation of the %s failed", RowsStage::what(bad));
        const int rc = stage.fill(c, B, V, rec.data(), lrows, grammar ? &g : nullptr, nullptr, st);
        if (stage.hip_err != hipSuccess) MGEA_CHECK_HIP(stage.hip_err);   // (as before the helper: this path does not synchronise)
        if (rc != MGEA_OK) return op_finish(rc, st);
        t.s.params = stage.rec_dev;
    }
    if (kind == 0) return op_finish(launch_argmax_advance(a->pval_dev, a->pidx_dev, a->n_tiles, t.s, a->sampled_dev, B, st), st);
    if (kind == 1) return op_finish(launch_argmax_advance_embed(a->pval_dev, a->pidx_dev, a->n_tiles, t, a->sampled_dev, B, st), st);
    if (kind == 2) {
        const ScoreFile f{a->logprob_step_dev, a->choice_step_dev, a->logprob_hist_dev, a->choice_hist_dev, a->hist_stride};
        return op_finish(launch_advance(a->sampled_dev, t.s, B, st, a->presence_dev, V, scored ? &f : nullptr), st);
    }
    if (kind == 3) return op_finish(launch_embed_qkv0(a->cur_ids_dev, a->ctx_len_dev, t, B, a->err_flag_dev, st), st);
    // kind 4: the sampler with its fused tail
    if (scored) c.score = ScoreArgs{a->forced_dev, a->forced_stride, a->logprob_hist_dev, a->choice_hist_dev, a->hist_stride, a->err_flag_dev};
    return op_finish(launch_sample(c, st), st);
}

int mgea_op_dec_embed(int32_t form, const int32_t* ids_dev, const int32_t* lens_dev, const int32_t* ctx_len_dev, const float* tok_emb_dev,
                      const float* pos_emb_dev, float* x_out_dev, float* aux_out_dev, const float* ln_w_dev, const float* ln_b_dev,
                      float eps, int32_t B, int32_t T, int32_t C, int32_t vocab, int32_t pos_rows, int32_t absolute_pos,
                      int32_t* err_flag_dev, void* stream) {
    MGEA_REQUIRE((form == 0 || form == 1) && ids_dev && tok_emb_dev && pos_emb_dev && x_out_dev && B > 0 && T > 0 && C > 0 && vocab > 0 &&
                     pos_rows > 0,
                 MGEA_EINVAL, "op_dec_embed: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (form == 0) {
        MGEA_REQUIRE(aux_out_dev, MGEA_EINVAL, "op_dec_embed: form 0 writes the statistics to aux_out_dev");
        MGEA_REQUIRE(C % 32 == 0 || (int64_t)B * T <= 64, MGEA_EINVAL, "op_dec_embed: a k-tiled x of width %d (no multiple of 32) holds at most 64 rows", C);
        return op_finish(launch_embed_stats(ids_dev, lens_dev, ctx_len_dev, tok_emb_dev, pos_emb_dev, x_out_dev, aux_out_dev, B, T, C, vocab,
                                            pos_rows, absolute_pos, err_flag_dev, st), st);
    }
    MGEA_REQUIRE(!ln_w_dev || (ln_b_dev && aux_out_dev), MGEA_EINVAL, "op_dec_embed: LayerNorm weights without ln_b_dev / aux_out_dev");
    return op_finish(launch_embed_ln(ids_dev, lens_dev, ctx_len_dev, tok_emb_dev, pos_emb_dev, x_out_dev, aux_out_dev, ln_w_dev, ln_b_dev, eps,
                                     B, T, C, vocab, pos_rows, absolute_pos, err_flag_dev, st), st);
}

int mgea_op_take_last(const int32_t* ids_dev, const int32_t* lens_dev, int32_t* cur_ids_dev, int32_t B, int32_t T, void* stream) {
    MGEA_REQUIRE(ids_dev && cur_ids_dev && B > 0 && T > 0, MGEA_EINVAL, "op_take_last: bad argument");
    return op_finish(launch_take_last(ids_dev, lens_dev, cur_ids_dev, B, T, (hipStream_t)stream), (hipStream_t)stream);
}

int mgea_op_add_lens(int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t T, int32_t B, void* stream) {
    MGEA_REQUIRE(ctx_len_dev && B > 0, MGEA_EINVAL, "op_add_lens: bad argument");
    return op_finish(launch_add_lens(ctx_len_dev, lens_dev, T, B, (hipStream_t)stream), (hipStream_t)stream);
}

int mgea_op_presence_seed(const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t V, uint32_t* presence_dev,
                          void* stream) {
    MGEA_REQUIRE(ids_dev && presence_dev && B > 0 && T > 0, MGEA_EINVAL, "op_presence_seed: bad argument");
    return op_finish(launch_presence_seed(ids_dev, lens_dev, B, T, V, presence_dev, (hipStream_t)stream), (hipStream_t)stream);
}

int mgea_op_unpark_rows(int32_t* done_dev, int32_t* ctx_len_dev, int32_t B, void* stream) {
    MGEA_REQUIRE(done_dev && ctx_len_dev && B > 0, MGEA_EINVAL, "op_unpark_rows: bad argument");
    return op_finish(launch_unpark_rows(done_dev, ctx_len_dev, B, (hipStream_t)stream), (hipStream_t)stream);
}

int mgea_op_grammar_allow(const int32_t* next_dev, int32_t n_state, int32_t n_class, uint32_t* allow_dev, void* stream) {
    MGEA_REQUIRE(next_dev && allow_dev, MGEA_EINVAL, "op_grammar_allow: NULL argument");
    return op_finish(launch_grammar_allow(next_dev, n_state, n_class, allow_dev, (hipStream_t)stream), (hipStream_t)stream);
}

int mgea_op_row_budgets(const mgea_sampler_config* s, const mgea_row_sampler* rows, int32_t B, const int32_t* lens_dev, int32_t T,
                        int32_t reserved, mgea_row_sampler* rows_out, int32_t* ctx_cap_out, void* stream) {
    MGEA_REQUIRE((s || rows) && B > 0 && T > 0 && reserved >= 0 && rows_out && ctx_cap_out, MGEA_EINVAL, "op_row_budgets: bad argument");
    MGEA_REQUIRE(reserved == 0 || T < reserved, MGEA_EINVAL, "op_row_budgets: prompt width %d leaves no room in %d tokens", T, reserved);
    hipStream_t st = (hipStream_t)stream;
    std::vector<SamplerParams> rec((size_t)B);
    SamplerParams* rec_dev = nullptr;
    DevGroup tmp;
    MGEA_REQUIRE(tmp.alloc(&rec_dev, (size_t)B * sizeof(SamplerParams)) == MGEA_OK, MGEA_ENOMEM, "op_row_budgets: allocation of the records failed");
    int rc = MGEA_OK;
    if (rows) {
        MGEA_TRY(check_row_samplers(rows, B, MGEA_SAMPLER_MAX_VOCAB, -1, "op_row_budgets"));
        build_row_records(rows, nullptr, B, -1, rec.data());
        MGEA_CHECK_HIP(hipMemcpyAsync(rec_dev, rec.data(), (size_t)B * sizeof(SamplerParams), hipMemcpyHostToDevice, st));
    } else {
        rc = launch_fill_sampler_params(rec_dev, sampler_params(*s), B, st);
    }
    if (rc == MGEA_OK && reserved > 0) rc = launch_clamp_budgets(rec_dev, lens_dev, T, B, reserved, st);
    if (rc == MGEA_OK && hipMemcpyAsync(rec.data(), rec_dev, (size_t)B * sizeof(SamplerParams), hipMemcpyDeviceToHost, st) != hipSuccess) {
        set_error("op_row_budgets: copy of the records failed");
        rc = MGEA_EHIP;
    }
    MGEA_TRY(op_finish(rc, st));
    for (int b = 0; b < B; ++b) {
        const SamplerParams& p = rec[b];
        rows_out[b] = mgea_row_sampler{p.temperature, p.top_k, p.top_p, p.penalty, p.eos_id, p.max_new,
                                       ((uint64_t)p.seed_hi << 32) | p.seed_lo, p.stream, 0u};
        ctx_cap_out[b] = p.ctx_cap;
    }
    return MGEA_OK;
}

}  // extern "C"

static int op_sample_rows(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                          const mgea_row_logits* lrows, int64_t step, int32_t* ids_out_dev, float* probs_out_dev, const ScoreArgs& score,
                          void* stream, const GrammarArgs* grammar, const mgea_row_truncation* trunc) {
    MGEA_REQUIRE(logits_dev && rows && B > 0, MGEA_EINVAL, "op_sample_rows: NULL argument or empty batch");
    MGEA_TRY(check_row_samplers(rows, B, V, -1, "op_sample_rows"));
    if (lrows) MGEA_TRY(check_row_logits(lrows, B, -1, "op_sample_rows"));
    int n_trunc = 0;
    if (trunc) MGEA_TRY(check_row_truncation(trunc, rows, B, "op_sample_rows_truncated", &n_trunc));
    std::vector<SamplerParams> rec((size_t)B);
    const RowRecords rr = build_row_records(rows, lrows, B, -1, rec.data());
    const bool biased = rr.form == StepForm::BIASED;
    MGEA_REQUIRE(!rr.any_penalty || presence_dev, MGEA_EINVAL, "op_sample_rows: a row is penalized but presence_dev is NULL");
    hipStream_t st = (hipStream_t)stream;
    // the grammar and the truncating form are built on the biased one: both bring the bias buffer, and empty bitmaps where none came
    RowsStage stage;   // nothing is enqueued before the allocations, and the stream is synchronised before they are freed
    const int bad = stage.alloc(B, V, true, biased || grammar || trunc, grammar, trunc != nullptr, presence_dev != nullptr);
    MGEA_REQUIRE(bad != RowsStage::RECORDS, MGEA_EHIP, "hipMalloc((void**)&rec_dev, (size_t)B * sizeof(SamplerParams)) failed: %s (%s:%d)",
                 hipGetErrorString(hipGetLastError()), __FILE__, __LINE__);
    MGEA_REQUIRE(!bad, MGEA_ENOMEM, "op_sample_rows: allocation of the %s failed", RowsStage::what(bad));
    SampleCall c = op_sample_call(logits_dev, B, V, step, ids_out_dev, probs_out_dev);
    // (a bias alone needs no bitmap here: nothing is written)
    c.presence = (rr.any_penalty || grammar || trunc) ? const_cast<uint32_t*>(presence_dev) : nullptr;
    c.score = score;
    int rc = MGEA_EHIP;
    if (stage.fill(c, B, V, rec.data(), biased ? lrows : nullptr, grammar, trunc, st) == MGEA_OK)
        rc = launch_sample(c, st);
    else
        set_error("op_sample_rows: copy of the records failed");
    const hipError_t e = hipStreamSynchronize(st);   // rec and the stage's buffers are freed on return
    MGEA_TRY(rc);
    MGEA_CHECK_HIP(e);
    return MGEA_OK;
}
