// Shared host/device helpers for the gfx950 kernels.  wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/mgea.h"
#include "gemm16_plan.h"
#include "gen_plan.h"   // GenRequest / StepKind / GenPlan, the rows' host checks, MGEA_REQUIRE / MGEA_TRY

namespace mgea {

// ---- error plumbing (thread-local message behind mgea_last_error) --------------------------
void set_error(const char* fmt, ...);
const char* get_error();

#define MGEA_CHECK_HIP(expr)                                                          \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            ::mgea::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                              __FILE__, __LINE__);                                    \
            return MGEA_EHIP;                                                         \
        }                                                                             \
    } while (0)

// ---- A/B and test switches (tools/README.md) ------------------------------------------------
// One process-global table, filled ONCE when the library is loaded from the MGEA_<NAME> environment variables and changed at
// run time only through mgea_tune_set() (tests, tools): nothing on a launch path reads the environment.
enum { TUNE_BF16_GEMM_TILE = 0,   // 0 = the launcher's choice; 1 128x128 / 2 256x128 / 3 256x256 ring kernels; 4 = the persistent 256x256 kernel
       TUNE_BF16_GEMM_SMALL,      // 1: the register-staged 128x128 kernel for every shape
       TUNE_BF16_GEMM_TAIL,       // persistent kernel, tiles left after the full rounds: 0 whole tiles, 1 two 128-row halves, 2 = 1 + staggered order
       TUNE_BF16_GEMM_PHASES,     // whole tiles of the persistent kernel: 4 phases of 16 MFMAs per K-tile, 2 (default) phases of 32, or 1 = software-pipelined, one barrier per K-tile
       TUNE_BF16_GEMM_REVERSE,    // 1 (default): the FFN down-projection walks its tiles from the end of each XCD's run (A = the up-projection's output)
       TUNE_BERT_BF16_NOFOLD,     // 1: bf16 DistilBERT with LayerNorm kernels instead of the folded-LayerNorm pipeline
       TUNE_DECODER_PREFILL_FULL, // 1: a decoder forward whose logits are dropped still runs the whole last block (default: it stops at that block's K | V)
       TUNE_BERT_FULL_LAST_LAYER, // 1: the last DistilBERT layer computes every position (as the reference does) instead of K | V for all + the rest for the [CLS] rows only
       TUNE_DECODER_UNFUSED, TUNE_DECODER_NOGEMV, TUNE_DECODER_NOGRAPH,   // read by mgea_decoder_create()
       TUNE_ATTN16_WIDE,          // 16-bit flash attention with 8 waves / 256-key stages: 0 never, 1 from 512 tokens on (default), 2 always
       TUNE_DECODER_PREFILL16_PAGES,     // 1 (default): the fp16 prefill writes K | V pages from inside its attention kernel (the rows are in LDS there); 0: a scatter kernel per layer re-reads them from the qkv buffer
       TUNE_DECODER_PREFILL16,    // fp16 engines, big-batch prefill: 0 keep the exact-fp32 kernels (A/B), 1 f16 matrix cores when the batch
                                  // fills the chip (default), 2 whenever the kernels accept the shape (tests)
       TUNE_HEAD_BALANCED,        // 1 (default): the LM head of a 3..64-row decode step on head_balanced_kernel (one workgroup per CU, equal unit counts); 0: the generic skinny kernel
       TUNE_ATTN16_PIPE,          // 1 (default): the 16-bit flash attention runs full key stages software-pipelined (next tile's Q K^T under this tile's exponentials); 0: rolled loop
       TUNE_SKINNY_ONE_PER_CU,    // 1: skinny GEMM launches of <= 256 workgroups ask for > 80 KB of LDS, so that no two share a CU (A/B; default 0)
       TUNE_SAMPLER_WAVE_SELECT,  // 1 (default): top_k <= 64 finds its boundary wave by wave (ballots only) and merges 4 x 64 candidates after one barrier; 0: block-wide bisection, a barrier per bit
       TUNE_ATTN_SPLIT,           // the decode step's attention of at most this many (row, head) pairs spreads each pair's KV pages over several workgroups, the last one to arrive merges their partials (default 64 = 8 rows of 8 heads: measured +3..5 % tokens/s at 1-8 rows, nothing at 16, -3.5 % at 32; 0: always one workgroup per pair)
       TUNE_DECODER_GRAPH_STEPS,  // decode steps per hipGraph launch of mgea_decoder_generate: 1, 2, 4, 8 (default) or 16; the single-step graph serves the remainder (round 4: 289.4 -> 287.6 us per step at B = 64, 168.3 -> 163.4 at B = 1)
       TUNE_ATTN_ARITH_PAGES,     // 1 (default): the decode attention computes physical page ids (j * batch + b, the decoder's own allocation) instead of loading them from the page table -- one dependent scalar load less per page; 0: always the table
       TUNE_DECODER_QKV0_TABLE,   // 1 (default): f32 engines in the reference's position mode keep layer 0's q | k | v of every token id in a [vocab][3 C] table and the step's tail gathers the row, so the layer-0 in-projection launch leaves the step (decoder_handle.h, "qkv0 table"; +vocab * 3 C * 4 bytes per engine and decode path); 0: the launch.  Read by mgea_decoder_create()
       TUNE_ATTN_CAUSAL_WALK,     // the causal dense attention's walk of its grid = the kernel's CAUSAL template value: 1 (default) (row, head) pairs fastest and blocks last to first, so that a pair's blocks share an XCD and its L2; 2 the non-causal kernel's order, block index fastest (attn_dense.hip; A/B: profiles/causal_prefill_ab.txt)
       TUNE_COUNT };
int tune(int key);

// per-device facts the launchers need (cached per device id; one process may drive several devices)
struct DeviceInfo { int dev; int n_cu; };
int device_info(DeviceInfo* out);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device): `done` is the instantiation's own bit mask
int set_max_dynamic_lds(const void* fn, int bytes, int dev, uint64_t* done);

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// "k-tiled" activation layout of the fused decode path, in MFMA-fragment order: a [<=64, N] matrix is cut
// into 32-wide k-chunks of 2048 floats; inside a chunk the 16-byte group holding (row, k..k+3) sits at
//   [row / 16][h = (k / 4) % 2][lane = (k / 8) % 4 * 16 + row % 16]
// which is exactly the order in which the 64 lanes of a wave consume it in the skinny GEMM (lane = 16 g + c
// feeds row c with k = k0 + 8 g + 4 h + s): one operand load instruction reads 1 KB of CONSECUTIVE bytes.
// Measured on MI355X: a wave load whose lanes each fetch 16 B from a different 128-B line is served at about
// one lane per clock (~16 B/clk, 36 GB/s per CU); consecutive lanes reach the 64 B/clk of the L1.
// Rows beyond 64 (decode batches of up to MGEA_FUSED_MAX_ROWS rows) continue in further 64-row groups of 64 * N floats each.
constexpr int MGEA_FUSED_MAX_ROWS = 512;
__host__ __device__ static inline int64_t tiled_off(int row, int n, int N) {
    const int r = row & 63;
    return (int64_t)(row >> 6) * 64 * N + (int64_t)(n >> 5) * 2048 +
           ((((r >> 4) * 2 + ((n >> 2) & 1)) * 64 + ((n >> 3) & 3) * 16 + (r & 15)) << 2) + (n & 3);
}
// The same idea for the weights of the skinny GEMMs (W [N, K] row-major in the arena): per (16-row tile,
// 32-wide k-chunk) one 2 KB block [h][lane = 16 g + c][4] holding W[tile * 16 + c][chunk * 32 + 8 g + 4 h + s];
// rows are padded to a multiple of 32 with zeros.  Built once per engine from the arena (launch_tile_weights).
static inline int64_t wtile_floats(int N, int K) { return round_up(N, 32) * (int64_t)K; }
int launch_tile_weights(const float* W, int N, int K, float* out, hipStream_t st, const float* gamma = nullptr);
// fp16 twin (MGEA_DTYPE_F16): per (16-row tile, 32-wide k-chunk) one 1 KB block [lane = 16 g + c][8] of _Float16 holding
// W[tile * 16 + c][chunk * 32 + 8 g + 0..7] -- the A/B fragment of v_mfma_f32_16x16x32_f16; out has wtile_floats(N, K) halves
int launch_tile_weights_f16(const float* W, int N, int K, void* out, hipStream_t st);
// c1[n] = sum_k gamma[k] * W[n,k], c2[n] = sum_k beta[k] * W[n,k] + bias[n] (fp64 sums of exact products): the folded-LayerNorm
// vectors when gamma is applied on the activation side (fp16 mode)
int launch_ln_vectors(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, float* c1, float* c2,
                      hipStream_t st);
// x[i] <- float(half(x[i])) in place (round-to-nearest-even): the fp16 engine's private fp32 copy of the matrices
int launch_round_f16_inplace(float* x, int64_t n, hipStream_t st);
// LayerNorm folded into the matrix it feeds: out = tiles of gamma[k] * W[n,k]; c1[n] = sum_k of those products,
// c2[n] = sum_k beta[k] * W[n,k] + bias[n] (sums in fp64, once per engine)
int launch_ln_fold(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, float* out,
                   float* c1, float* c2, hipStream_t st);
// row-major [M, N] <-> k-tiled (to_tiled != 0: src row-major, dst tiled), for tests and tools
int launch_tile_rows(const float* src, float* dst, int M, int N, int to_tiled, hipStream_t st);

// ---- kernel launchers (defined in the .hip files) -------------------------------------------

// P[z][M, ldp] = A[M, k-slice z] @ W[N, k-slice z]^T   (raw partial products, no bias)
// ldp = round_up(N, 64); slab stride = M * ldp floats.  K % 32 == 0.
int launch_gemm_f32(const float* A, int lda, const float* W, int ldw, float* P, int M, int N, int K,
                    int split_k, hipStream_t st);
int launch_gemm_f32_bias_act(const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldo,
                             int M, int N, int K, int act, hipStream_t st);
// chooses split_k so the grid fills the chip (deterministic function of the shape)
int pick_split_k(int M, int N, int K, int64_t cap_floats = -1);   // cap: slab workspace of the caller (floats)
bool gemm_direct_epilogue_ok(int M, int N);
static inline int64_t slab_ld(int N) { return round_up(N, 64); }
static inline int64_t slab_floats(int M, int N) { return (int64_t)M * slab_ld(N); }

// Row epilogues over S slabs P (slab stride `ps`, leading dim `ldp`): v = sum_s P[s][m][n] + bias[n]
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };
// out[m, n] = act(v)
int launch_bias_act(const float* P, int S, int64_t ps, int ldp, const float* bias, float* out, int ldo,
                    int M, int N, int act, hipStream_t st);
// pre-LN :  x += v;  xn = LN(x; lnw, lnb) (xn written only if lnw != NULL)
// post-LN:  x = LN(x + v; lnw, lnb)
int launch_bias_res_ln(const float* P, int S, int64_t ps, int ldp, const float* bias, float* x, float* xn,
                       const float* lnw, const float* lnb, float eps, int M, int C, int post_ln,
                       hipStream_t st);
int launch_layernorm(const float* x, const float* w, const float* b, float* y, int M, int C, float eps,
                     hipStream_t st);

// Paged KV pool: [n_layer][n_pages][K | V][H][one page = 64 tokens x dh elements]; elements are fp32 (parity mode) or
// fp16 (MGEA_DTYPE_F16).  Inside a page, with G = the elements of one 16-byte group (4 floats / 8 halves):
//   K: [dh / G][64 tokens][G]  (token-major inside a d-group: in the decode kernel lane = token, every wave load
//                               instruction is 1 KiB of consecutive bytes)
//   V: [64 tokens][dh]         (a wave instruction reads 1 KiB = several whole rows)
struct KvPool {
    void* base;
    int32_t n_pages;      // physical pages per layer
    int32_t H, dh;
    int32_t spare;        // (the word the alignment of layer_stride leaves free, named so that a kernel can list it with the rest: SkinnyArgs)
    int64_t layer_stride; // elements
    int32_t f16;          // 0: float elements, 1: _Float16 elements
    int32_t arith_batch;  // > 0: the page table holds logical page j of row b -> physical j * arith_batch + b (what mgea_decoder_reset
                          // writes): a kernel may compute that instead of loading it; 0: only the table says
    __host__ __device__ int64_t page_elems() const { return (int64_t)MGEA_KV_PAGE_TOKENS * dh; }
    __host__ __device__ int elt_bytes() const { return f16 ? 2 : 4; }
};

// decoder embedding: x[m] = tok_emb[ids[m]] + pos_emb[pos]; xn = LN(x) if lnw.
// rows m = b*T + t; rows with t >= lens[b] are zero-filled.  pos = t (+ ctx_len[b] if absolute).
// err_flag (device int32 or NULL): bit 0 is set when a real token id lies outside [0, vocab) (it is clamped).
int launch_embed_ln(const int32_t* ids, const int32_t* lens, const int32_t* ctx_len, const float* tok_emb,
                    const float* pos_emb, float* x, float* xn, const float* lnw, const float* lnb, float eps,
                    int B, int T, int C, int vocab, int pos_rows, int absolute_pos, int32_t* err_flag, hipStream_t st);
// BERT embedding: h[m] = LN(word[ids[m]] + pos[t])
int launch_bert_embed_ln(const int32_t* ids, const float* word, const float* pos, const float* lnw,
                         const float* lnb, float eps, float* h, int B, int S, int D, int vocab,
                         hipStream_t st, int32_t* err_flag = nullptr, const int32_t* pos_ids = nullptr);   // pos_ids: packed rows (B = rows, S = 1)
// qkv epilogue of the decoder: v = sum P + bias over [M, 3C]; q -> qbuf[m, C] (and k|v -> kvbuf
// [m, 2C] if kvbuf != NULL, for the no-cache attention); k, v of real tokens -> KV pages of `layer`
// at position ctx_len[b] + t.
int launch_qkv_scatter(const float* P, int S, int64_t ps, int ldp, const float* bias, float* qkv_out,
                       const KvPool& pool, int layer, const int32_t* page_table, int max_pages,
                       const int32_t* ctx_len, const int32_t* lens, int B, int T, int C, hipStream_t st);
// decode / extend attention over the paged cache: query rows m = b*T + t attend to
// ctx_len[b] + (lens ? lens[b] : T) cached tokens.  q read from qkv[m, 0:C] (row stride 3C).
// split (small batches): scratch of the split-context form -- part [max_items][max_split][attn_part_floats(dh)] floats, count
// [max_items] int32 zeroed once (the kernel leaves them zero); NULL, or a shape attn_split_count() answers 1 for: one workgroup per
// (row, head, query).
constexpr int MGEA_ATTN_MAX_SPLIT = 16, MGEA_ATTN_SPLIT_ITEMS = 256;
__host__ __device__ constexpr int attn_part_floats(int dh) { return dh + 2; }   // acc[dh], max, sum
struct AttnSplit { float* part; int32_t* count; int max_split, max_items; };
int attn_split_count(int B, int H, int T, int max_pages);
int launch_attn_paged(const float* qkv, const KvPool& pool, int layer, const int32_t* page_table,
                      int max_pages, const int32_t* ctx_len, const int32_t* lens, float* out, int B, int T,
                      int C, int tiled_out, hipStream_t st, const AttnSplit* split = nullptr, int causal = 0);
// causal != 0 with T > 1: query (b, t) sees ctx_len[b] + t + 1 tokens, not all T new ones (T == 1: the same launch either way)
// dense non-causal attention over the qkv buffer itself (prefill without past, BERT)
int launch_attn_dense(const float* qkv, const int32_t* lens, const int32_t* mask, float* out, int B, int T,
                      int H, int dh, int tiled_out, hipStream_t st, const int32_t* cu = nullptr, int causal = 0);   // cu: packed rows (T = the longest sequence)
// causal != 0: query i sees the keys t <= i with t < lens[b]; refuses mask and cu

// The sampler's scalars as the kernels read them from DEVICE memory: one 48-byte record per row, [max_batch] per engine.  A captured
// decode-step graph holds only the pointer, so one graph serves every request whatever its seed / temperature / top-k / top-p / EOS id
// (mgea_sampler_config, api_cache.py:160,204) -- and a batch whose rows carry different ones (mgea_decoder_generate_rows).
// penalty: the repetition penalty of a penalized generation (read only by the PENALTY sampler; 1 otherwise).
// stream: word 0 of the row's Philox counter (the key is the seed); generate() writes stream = b.
// max_new: the row's step budget -- it finishes after producing that many tokens (end_row_step); INT32_MAX = none.
// ctx_cap: the tokens the row's KV pages hold when that is less than the longest prompt + the steps (launch_clamp_budgets); INT32_MAX = none.
// bias_on: the row adds its row of the bias buffer to its logits; min_new: no eos_id before the row has produced that many ids (both
// read only by the BIAS sampler; 0 otherwise).
struct SamplerParams {
    float temperature; int32_t top_k; float top_p; int32_t eos_id;
    uint32_t seed_lo, seed_hi; float penalty; uint32_t stream;
    int32_t max_new; int32_t ctx_cap; int32_t bias_on; int32_t min_new;
};
constexpr int32_t MGEA_NO_BUDGET = 0x7fffffff;
static inline SamplerParams sampler_params(const mgea_sampler_config& s, float penalty = 1.0f) {
    return SamplerParams{s.temperature, s.top_k, s.top_p, s.eos_id, (uint32_t)s.seed, (uint32_t)(s.seed >> 32), penalty, 0u,
                         MGEA_NO_BUDGET, MGEA_NO_BUDGET, 0, 0};
}
// a per-row record of the C ABI -> the device record (max_new_tokens 0 = no budget: the call's n_steps bound the row anyway)
static inline SamplerParams sampler_params(const mgea_row_sampler& r) {
    return SamplerParams{r.temperature, r.top_k, r.top_p, r.eos_id, (uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.repetition_penalty,
                         r.stream, r.max_new_tokens > 0 ? r.max_new_tokens : MGEA_NO_BUDGET, MGEA_NO_BUDGET, 0, 0};
}
// checked rows [B] (+ lrows [B] or NULL) -> out[B]; the batch's form and flags are row_records' (gen_plan.h, with the rows' host checks)
RowRecords build_row_records(const mgea_row_sampler* rows, const mgea_row_logits* lrows, int B, int n_steps, SamplerParams* out);
constexpr int MGEA_SAMPLER_MAX_VOCAB = 14336;   // the sampler keeps a row in registers: 256 threads x 56 logits
// Repetition penalty (mgea_decoder_generate_penalized): per row a presence bitmap of ceil(V / 32) words, bit id & 31 of word id >> 5
// set once the id is in the row's prompt or was generated by it.  Rows follow each other at that stride.
__host__ __device__ static inline int presence_words(int V) { return (V + 31) >> 5; }

// logits row epilogue: v = sum P + bias; optional store to logits[m, V]; greedy argmax path writes
// next ids and advances the per-row state (see decoder.hip).
struct StepState {
    int32_t* cur_ids;   // [B] token fed to the next step
    int32_t* ctx_len;   // [B]
    int32_t* done;      // [B]
    int32_t* row_step;  // [B] index of the step each row is producing (also the Philox counter)
    int32_t* n_done;    // [1]
    int32_t* ids_out;   // [B, n_steps] or NULL
    int32_t  n_steps;
    int32_t  eos_id;            // used when params == NULL (no budget then)
    const SamplerParams* params;   // [B] device records: row b's eos_id and max_new win (NULL: eos_id above)
};
// one query per sequence (the [CLS] position, fp32 q [B, D]) against the K | V columns of a packed qkv buffer [B * S, 3 D] (fp32 or bf16) -> fp32 [B, D]
int launch_attn_cls(const float* q, const void* qkv, int qkv_bf16, const int32_t* mask, float* out, int B, int S, int H, int dh, hipStream_t st,
                    const int32_t* cu = nullptr);
int launch_logits_argmax(const float* P, int S, int64_t ps, int ldp, const float* bias, float* logits,
                         int M, int V, int32_t* argmax_out, hipStream_t st);
// The fused tail of the sampler: it also does the loop bookkeeping of the row and the NEXT step's embedding (advance_embed_row)
struct TailArgs {
    StepState s;
    const float* tok_emb; const float* pos_emb;
    float* x; float* stats;     // k-tiled residual stream and its LayerNorm partials (fused decode path)
    int C, vocab, pos_rows, absolute_pos;
    // qkv0 != NULL (decoder_handle.h, "qkv0 table"): row [id] of the [vocab][3 C] table is layer 0's q | k | v of the embedding, so the tail also
    // does what the next step's layer-0 in-projection launch would have done -- the row into qkv [B][3 C], its K | V into layer 0's page --
    // and leaves out the embedding's LayerNorm statistics, which only that launch read.
    const float* qkv0; float* qkv;
    KvPool pool; const int32_t* page_table; int max_pages;
};
constexpr int QKV0_MAX_C = 1024;   // embed_qkv0_row moves a row with one float4 per thread of 256 (the fused geometry's d_model limit)
static inline bool tail_qkv0_ok(const TailArgs& t) {
    return !t.qkv0 || (t.qkv && t.pool.base && !t.pool.f16 && t.C % 4 == 0 && t.C <= QKV0_MAX_C && t.C % t.pool.dh == 0);
}
// What the scored sampler reads and writes besides the draw (sampler.hip, sample_kernel<..., ScoreArgs>).
// forced: ids the rows must take, -1 = the draw decides -- forced[b] when forced_stride == 0, else forced[b * forced_stride + step] for
// the row's step index (steps at or beyond the stride are free); NULL: nothing is forced.
// logprob / choice (choice may be NULL): with a fused tail the histories [B][out_stride], filed at the row's step; without one [B].
// err_flag (or NULL): bit 0 is set when a forced id >= vocab was clamped.
struct ScoreArgs {
    const int32_t* forced; int forced_stride;
    float* logprob; float* choice; int out_stride;
    int32_t* err_flag;
};
// A token grammar (mgea_decoder_set_grammar): a finite automaton over token classes, one per engine, shared by the rows.
//   class_of [V]                      the class of every id
//   next     [n_state][n_class]       the state after an id of that class, -1 = the class is banned in the state
//   allow    [n_state][words]         bit c & 31 of word c >> 5 of row s set iff next[s][c] >= 0 (launch_grammar_allow), words =
//                                     grammar_words(n_class) <= MGEA_GRAMMAR_MAX_WORDS: what the sampler stages in LDS
//   state_in / state_out [B]          the rows' states, -1 = the row has no grammar (the engine passes one array as both)
//   done [B] or NULL                  the rows' finished flags: a finished row is neither masked nor moved
//   err_flag or NULL                  bit 1 is set when the id a row takes is banned in its state (only a forced id can be); the state stays
// The GRAMMAR sampler masks x[i] = -inf where the row's state bans class_of[i] -- after the penalty and the bias, before the EOS ban --
// and its thread 0 stores next[state][class_of[id]] for the id the step commits.
constexpr int MGEA_GRAMMAR_MAX_CLASSES = 4096, MGEA_GRAMMAR_MAX_STATES = 4096, MGEA_GRAMMAR_MAX_CELLS = 1 << 20;
constexpr int MGEA_GRAMMAR_MAX_WORDS = MGEA_GRAMMAR_MAX_CLASSES / 32;
__host__ __device__ static inline int grammar_words(int n_class) { return (n_class + 31) >> 5; }
struct GrammarArgs {
    const int32_t* class_of; const int32_t* next; const uint32_t* allow;
    const int32_t* state_in; int32_t* state_out; const int32_t* done;
    int32_t n_state, n_class, words;
    int32_t* err_flag;
};
// The rows' truncation records (mgea_row_truncation, include/mgea.h: the rule), device [B]: the truncating sampler applies min-p,
// typical-p, the epsilon and the eta cutoff, in this order, to what top-k and top-p kept.  A row whose record switches nothing on, and
// a top_k == 1 row, skip all of it (block-uniform) and compute what the form computes without the argument.
struct TruncArgs { const mgea_row_truncation* rows; };
// allow[s][w] from next [n_state][n_class] (step_tail.hip)
int launch_grammar_allow(const int32_t* next, int n_state, int n_class, uint32_t* allow, hipStream_t st);
// The unfused path's second half: advance_kernel files the sampler's per-step values at the row's step (0 for a finished row).
struct ScoreFile { const float* logprob_step; const float* choice_step; float* logprob_hist; float* choice_hist; int stride; };
// One sampler launch over logits [B, V] (sampler.hip); every optional part is a named field, NULL = absent.
struct SampleCall {
    const float* logits; int B, V;
    // the scalars: the rows' device records (Philox counter word 0 = the record's stream), or `params` by value on every row
    // (sampler_params(s, penalty); counter word 0 = b).  With records, or in the PENALTY / BIAS forms, a row with top_k == 1 takes the
    // exact argmax of its processed row: no temperature division, ties to the lowest id.
    const SamplerParams* params_dev; SamplerParams params;
    // the step index (Philox counter word 1; what min_new is compared with): per row from device memory, or step_host
    const int32_t* row_step_dev; int64_t step_host;
    int32_t* ids_out; float* probs_out;   // [B] (NULL: nothing is drawn); [B, V] pre-draw probabilities
    const TailArgs* tail;                 // the fused tail; NULL: the sampler only writes ids_out
    // PENALTY form: the logits of the ids set in the row's bitmap (presence_words(V) words per row) are penalized first, x < 0 ? x * p :
    // x / p; a fused tail then adds the row's new token to the bitmap.  BIAS form (records only): after the penalty, row b adds
    // bias[b * V + i] to logit i if its record has bias_on, and bans its eos_id while its step index is below the record's min_new
    uint32_t* presence; const float* bias;
    // scored form (score.logprob != NULL): the raw and the choice log-probability of the id the row takes, and forced ids (ScoreArgs)
    ScoreArgs score;
    // GRAMMAR form (grammar.class_of != NULL; needs records, presence and bias): the rows' automaton (GrammarArgs)
    GrammarArgs grammar;
    // truncating form (trunc.rows != NULL; needs records, presence and bias): the rows' min-p / typical-p / epsilon / eta records (TruncArgs)
    TruncArgs trunc;
};
int launch_sample(const SampleCall& c, hipStream_t st);
// Classifier-free guidance between paired rows of logits [B, V], in place (guidance.hip): for every row c with u = partner[c] in [0, B),
// g = scale[c] * log_softmax(row c) + (1 - scale[c]) * log_softmax(row u) goes into BOTH rows; rows with partner < 0 that are nobody's
// partner stay as they are.  partner / scale: device [B].  The caller guarantees that no row is the partner of two rows and that a
// partner has no partner itself (one workgroup per pair is then the only one that touches its two rows).
int launch_guidance_mix(float* logits, int B, int V, const int32_t* partner, const float* scale, hipStream_t st);
// Emotion blends between grouped rows of logits [B, V], in place (blend.hip): for every row L with leader[L] == L, the rows b with
// leader[b] == L in ascending order m_0 < ... < m_{K-1} give g = sum_k weight[m_k] * log_softmax(row m_k) (added in that order), which
// goes into ALL K rows; rows whose leader is < 0 stay as they are.  leader / weight: device [B].  The caller guarantees that a named
// leader names itself and that a group has at most MGEA_BLEND_MAX_ROWS rows (one workgroup per group is then the only one that touches
// its rows).
int launch_blend_mix(float* logits, int B, int V, const int32_t* leader, const float* weight, hipStream_t st);
// Windowed penalties over token classes on logits [B, V], in place (class_penalty.hip; the rule: include/mgea.h, mgea_row_class_penalty):
// row b, not finished and with recs[b] on, counts the classes class_of[.] of hist[b * stride + j], j in the last recs[b].window of
// [0, row_step[b]), and subtracts frequency * n_c + presence from every id of a counted class.  class_of [V] in [-1, n_class); recs,
// row_step, done: device [B].  The caller guarantees row_step[b] <= stride.
int launch_class_penalty(float* logits, int B, int V, const int32_t* class_of, int n_class, const int32_t* hist, int stride,
                         const int32_t* row_step, const int32_t* done, const mgea_row_class_penalty* recs, hipStream_t st);
// Emotion transitions (recondition.hip; the rule and the store's layout: include/mgea.h, mgea_row_schedule / mgea_op_recondition).
// gather: positions [0, lens[b]) (lens NULL: Tp) of logical page 0 of every row, layer and head -> the slots of segment `seg` of the
// conditioning store, and the layout words / the rows' lengths -> meta [4] / cond_len [B].  apply: the launch that opens a scheduled
// decode step; rows whose segment changes get the new variant's positions back over their pages.  cond_store_bytes: the store's size.
int64_t cond_store_bytes(const KvPool& pool, int n_layer, int n_seg_max, int B, int slot_tokens);
int launch_cond_gather(const KvPool& pool, int n_layer, const int32_t* page_table, int max_pages, const int32_t* lens, int Tp, void* store,
                       int seg, int n_seg_max, int slot_tokens, int32_t* meta, int32_t* cond_len, int B, hipStream_t st);
int launch_cond_apply(const KvPool& pool, int n_layer, const int32_t* page_table, int max_pages, const void* store, const int32_t* meta,
                      const int32_t* cond_len, const mgea_row_schedule* sched, const int32_t* done, const int32_t* row_step,
                      const int32_t* gram_state, int32_t* cur_seg, int32_t* switches, int B, hipStream_t st);
// ---- the kernels that end a step, and the rows' records (step_tail.hip) ----
int launch_argmax_advance(const float* pval, const int32_t* pidx, int n_tiles, const StepState& s, int32_t* sampled,
                          int B, hipStream_t st);
int launch_argmax_advance_embed(const float* pval, const int32_t* pidx, int n_tiles, const TailArgs& t, int32_t* sampled, int B,
                                hipStream_t st);
// x, qkv and layer 0's K | V of ids[0, B) at the rows' ctx_len through the qkv0 table (t.qkv0 != NULL): what launch_embed_stats and the
// layer-0 in-projection launch leave, without the statistics; ids outside the vocabulary are clamped and flagged as there
int launch_embed_qkv0(const int32_t* ids, const int32_t* ctx_len, const TailArgs& t, int B, int32_t* err_flag, hipStream_t st);
// params_dev[0, B) <- v with stream = b, stream-ordered: the uniform form of the records
int launch_fill_sampler_params(SamplerParams* params_dev, const SamplerParams& v, int B, hipStream_t st);
// params_dev[b].max_new <- min(max_new, reserved - len_b), len_b = lens[b] (NULL: T) clamped to [1, T], and ctx_cap <- reserved: a row
// stops where its KV pages end
int launch_clamp_budgets(SamplerParams* params_dev, const int32_t* lens, int T, int B, int reserved, hipStream_t st);
// after a generation with capped rows: done 2 (parked, end_row_step) -> 1 with ctx_len + 1
int launch_unpark_rows(int32_t* done, int32_t* ctx_len, int B, hipStream_t st);
// after ids for this step are in `sampled` [B]: apply EOS/done logic, write ids_out[b, step],
// cur_ids, ctx_len += 1, row_step += 1; presence != NULL (bitmap of presence_words(V) words per row): also set the bit of the
// token of every row that was not finished yet
// score != NULL: also file the step's log-probabilities (ScoreFile)
int launch_advance(const int32_t* sampled, const StepState& s, int B, hipStream_t st, uint32_t* presence = nullptr, int V = 0,
                   const ScoreFile* score = nullptr);
// presence rows [0, B) <- the set of the real tokens of ids [B, T] (lens: first lens[b] of row b, NULL: all T; ids outside [0, V) skipped)
int launch_presence_seed(const int32_t* ids, const int32_t* lens, int B, int T, int V, uint32_t* presence, hipStream_t st);
// The first launch of a windowed decode step (kv_window.hip; the contract: include/mgea.h, mgea_decoder_set_window): a row that is not
// finished and has ctx_len == 64 (S + R) - 1 rotates page_table[b][S .. S+R-1] left by one, ctx_len - 64, evictions + 1.
constexpr int WINDOW_MAX_RING = 256;   // the ring of a row is held in registers: 4 entries per lane of one wave
int launch_window_evict(int32_t* page_table, int max_pages, int S, int R, int32_t* ctx_len, const int32_t* done, int32_t* evictions,
                        int B, hipStream_t st);
// ctx_len[b] += (lens ? lens[b] : T)
int launch_add_lens(int32_t* ctx_len, const int32_t* lens, int T, int B, hipStream_t st);
// cur_ids[b] = ids[b, (lens ? lens[b] : T) - 1]
int launch_take_last(const int32_t* ids, const int32_t* lens, int32_t* cur_ids, int B, int T, hipStream_t st);
// lens_m1[b] = (lens ? lens[b] : T) - 1, never below 0: what a causal engine prefills of a prompt (its last token is fed by the first step)
int launch_lens_minus_one(const int32_t* lens, int32_t* lens_m1, int T, int B, hipStream_t st);
// out[m] = logits[m][targets[m]] - logsumexp(logits[m]) over V entries of a row of stride ld; targets[m] < 0 gives 0, >= V clamps
int launch_logprob_gather(const float* logits, int64_t ld, const int32_t* targets, float* out, int M, int V, hipStream_t st);
int launch_gather_rows(const float* src, int ld_src, float* dst, int ld_dst, int rows, int row_step, int C,
                       hipStream_t st, const int32_t* row_idx = nullptr);   // row_idx: source row of output row r (instead of r * row_step)
int launch_lora_merge(float* w, const float* a, const float* b, int out_dim, int in_dim, int r, float scale,
                      hipStream_t st);

// ---- 16-bit perf-mode kernels (gemm16.hip, attn16.hip, rows16.hip); bf16 / fp16 buffers travel as void* ------
int launch_f32_to_bf16(const float* src, void* dst, int64_t n, hipStream_t st, int f16 = 0);   // f16: _Float16 instead of bf16
// C = epi(A @ W^T + bias), epi = a BEPI_* of gemm16_plan.h: 0 bias, 1 bias + GELU, 2 bias + residual(res, ld = ldc)
// LayerNorm folded around the 16-bit GEMMs (gemm16.hip, epilogues 3-5 of launch_gemm_bf16; persistent 256 x 256 kernel only).
//   epi 3 / 4 (LNFOLD / +GELU): A = RAW rows, W = W diag(gamma) in bf16, c1[n] = sum_k W'[n, k], bias slot = c2 = b + W beta;
//                               rowstat = (mean, rstd) of the A rows, [M][2]; out = rstd (A W'^T - mean c1) + c2
//   epi 5 (RES_LN): out = A W^T + bias + LayerNorm(res row) with the residual's rowstat / ln_g / ln_b (an already normalised
//                   residual comes with identity tables: mean 0, rstd 1, gamma 1, beta 0); stats_out (or nullptr) receives (sum, M2 =
//                   sum of squared deviations from the tile's own mean) of every output row per 256-column tile, [M][N / 256][2],
//                   from which launch_ln_rowstat makes the next (mean, rstd).
struct BfEpiLn { const float* rowstat; const float* c1; const float* ln_g; const float* ln_b; float* stats_out; };
// What a launch_gemm_bf16 call ran, from its plan (optional out-parameter; the engines count these for mgea_bert_stats): kernel = the
// G16_* family (0 the register-staged 128 x 128 kernel, 1 a ring kernel, 2 the persistent phase-interleaved 256 x 256 kernel, 3 the
// two-workgroups-per-CU 256 x 128 kernel, switch bf16_gemm_tile = 5 only); half_tiles = 1 when the persistent kernel cuts the tiles
// left over after its full rounds into two 128-row halves (gemm16.hip, "HALF-TILE TAIL"); tail_mode = the persistent kernel's tail word
// (Gemm16Plan.tail_mode: bits 0-1 the tail schedule, bit 2 the reversed walk; 0 for the other families).
struct GemmBf16Info { int kernel; int half_tiles; int tail_mode; };
// f16 != 0: _Float16 operands / outputs (persistent kernel, epilogues 3 / 4 / 5, and 6 = fp32 output).  reverse != 0: ask the persistent
// kernel to walk its tiles from the end of every XCD's run (switch bf16_gemm_reverse; for a GEMM whose A operand is the previous
// kernel's large output: see the kernel).
int launch_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res, void* C,
                     int ldc, int M, int N, int K, int epi, hipStream_t st, GemmBf16Info* info = nullptr, const BfEpiLn* ln = nullptr,
                     int f16 = 0, int reverse = 0);
// true when launch_gemm_bf16 would run this shape on the persistent 256 x 256 kernel (the only one with epilogues 3-5)
bool gemm_bf16_is_persistent(int M, int N, int K);
int launch_ln_rowstat(const float* part, float* rowstat, int M, int n_part, int C, float eps, hipStream_t st);
int launch_fold_ln_weights_bf16(const float* W, const float* gamma, const float* beta, const float* b, void* Wf, float* c1, float* c2,
                                int N, int K, hipStream_t st, int f16 = 0);
// cu (here and below; NULL = padded [B, S] rows): packed input, the rows of sequence b are cu[b] .. cu[b + 1] - 1
int launch_gather_cls_ln_bf16(const void* h, const float* rowstat, const float* g, const float* be, float* out, int B, int S, int D,
                              hipStream_t st, const int32_t* cu = nullptr);
int launch_layernorm_bf16(const void* x, const float* w, const float* b, void* y, int M, int C, float eps, hipStream_t st);
int launch_bert_embed_ln_bf16(const int32_t* ids, const float* word, const float* pos, const float* lnw, const float* lnb,
                              float eps, void* h, int B, int S, int D, int vocab, hipStream_t st, int32_t* err_flag = nullptr,
                              const int32_t* pos_ids = nullptr);
int launch_gather_cls_bf16(const void* h, float* out, int B, int S, int D, hipStream_t st, const int32_t* cu = nullptr);
// pages (fp16 instantiation only, or NULL): the K | V rows of every key whose mask bit is set also go to the fp16 KV pages of `layer` at
// position t (decoder prefill into an empty cache: the attention kernel has those rows in LDS anyway)
struct KvPages { KvPool pool; int layer; const int32_t* page_table; int max_pages; };
int launch_attn_bf16(const void* qkv, const int32_t* mask, void* out, int B, int T, int H, int dh, hipStream_t st, int f16 = 0,
                     const KvPages* pages = nullptr, const int32_t* cu = nullptr);

// fp16 big-batch prefill of the decoder (rows16.hip): embedding rows as fp16 + their (mean, rstd); K | V of fp16 qkv rows -> fp16 KV pages
int launch_dec_embed_f16(const int32_t* ids, const int32_t* lens, const int32_t* ctx_len, const float* tok_emb, const float* pos_emb,
                         void* x, float* rowstat, int32_t* mask_out, float eps, int B, int T, int C, int vocab, int pos_rows,
                         int absolute_pos, int32_t* err_flag, hipStream_t st);
int launch_kv_scatter_f16(const void* qkv, const KvPool& pool, int layer, const int32_t* page_table, int max_pages, const int32_t* ctx_len,
                          const int32_t* lens, int B, int T, int C, hipStream_t st);

// ---- fused skinny GEMM (decode step, M <= MGEA_FUSED_MAX_ROWS): gemm_skinny.hip --------------------------------
enum { EPI_QKV = 0, EPI_RES = 1, EPI_ACT = 2, EPI_LOGITS = 3 };

struct SkinnyArgs {
    // Field order is part of the kernels' prologue: what a decode launch reads comes first, without a hole, in the order of the
    // 64-byte lines of the kernel-argument block -- lines 0 and 1 for every epilogue, lines 2 and 3 for the QKV scatter.  The kernels
    // name every one of these fields in front of their first instruction, so the compiler fetches the lines with one batch of scalar
    // loads and one wait; a field it does not need, or a padding word, inside a wide load is a register it reuses at once, and the
    // load that reuses it has to wait for the first batch to land (tools/prologue_chain.py shows the batches of the compiled kernels).
    // ---- line 0
    const float* A;
    const float* W;            // [N, K] in the tiled weight layout (launch_tile_weights); fp16 tiles (launch_tile_weights_f16) if w_f16
    const float* bias;         // [N] or NULL
    float* out;                // QKV: qkv_out [M, N]; RES: x [M, N] (in place); ACT: out [M, ldo]; LOGITS: logits or NULL
    int M, N, K; int ldo;
    // folded LayerNorm (ln_c1 != NULL): W holds gamma * W, ln_c1 [N] = its row sums, bias = beta @ W^T + bias
    // (launch_ln_fold); per-row partial stats [64][n_part][2], each over `part_cnt` elements
    const float* ln_c1; const float* stats_in;
    // ---- line 1
    float eps; int n_part; int part_cnt;
    float inv_n_part, inv_k;   // 1 / n_part and 1 / (n_part * part_cnt), filled by the launcher (no division in the kernel)
    int act;
    int dbg;                   // ablation bits for tools/skinny_bench.py (0 in production)
    int nw;                    // waves per workgroup (set by the launcher)
    float* stats_out;          // RES: [64][N/16][2]
    const float* ln_g;         // gemv: LayerNorm gamma applied directly (W row-major, unfolded); w_f16 with ln_c1: gamma is applied
                               // to A on load (W stays the plain rounded matrix, ln_c1 = sum_k gamma_k W[n,k], bias = sum_k beta_k W[n,k] + b[n])
    float* pmax_val; int32_t* pmax_idx;   // LOGITS: [M][n_partials] (DecodeGemmPlan)
    // ---- lines 2 and 3: QKV scatter
    KvPool pool; int layer; int max_pages; const int32_t* page_table; const int32_t* ctx_len;
    const int32_t* lens; int T; int C;
    // ---- what no decode GEMM kernel reads from the block
    int lda;
    int w_f16;                 // MGEA_DTYPE_F16 engines: W holds _Float16 fragments, A is rounded to fp16 on load, f16 MFMA, fp32 accumulate
    const float* ln_b;         // gemv: LayerNorm beta applied directly
};

// lines 0 and 1 / lines 2 and 3 of the block as operands of an empty asm statement: every field is then in a scalar register in front of it
#define MGEA_SKINNY_ARGS_01(a) "s"((a).A), "s"((a).W), "s"((a).bias), "s"((a).out), "s"((a).M), "s"((a).N), "s"((a).K), "s"((a).ldo), \
    "s"((a).ln_c1), "s"((a).stats_in), "s"((a).eps), "s"((a).n_part), "s"((a).part_cnt), "s"((a).inv_n_part), "s"((a).inv_k), "s"((a).act), \
    "s"((a).dbg), "s"((a).nw), "s"((a).stats_out), "s"((a).ln_g), "s"((a).pmax_val), "s"((a).pmax_idx)
#define MGEA_SKINNY_ARGS_23(a) "s"((a).pool.base), "s"((a).pool.n_pages), "s"((a).pool.H), "s"((a).pool.dh), "s"((a).pool.spare), "s"((a).pool.layer_stride), \
    "s"((a).pool.f16), "s"((a).pool.arith_batch), "s"((a).layer), "s"((a).max_pages), "s"((a).page_table), "s"((a).ctx_len), "s"((a).lens), \
    "s"((a).T), "s"((a).C)

// ---- decode GEMMs: one launch plan per call (gemm_skinny.hip) ----------------------------------------------------
// Three kernel families serve them: gemm_skinny_kernel (tiled, LayerNorm-folded operands), head_balanced_kernel (head_gemm.hip:
// the LM head as one round of the chip) and gemv_rows_kernel (gemv_small.hip: <= 2 rows on the ROW-MAJOR weights, LayerNorm applied
// directly from ln_g / ln_b).  plan_decode_gemm makes every choice -- family, template parameters, geometry, the LOGITS partial
// count -- and launch_decode_gemm launches exactly that plan.
enum { DG_SKINNY = 0, DG_HEAD = 1, DG_GEMV = 2 };
struct DecodeGemmPlan {
    int kind;
    int mt, nt, nw;          // skinny: gemm_skinny_kernel<epi, ln, mt, nt, f16, nch>, nw waves per workgroup
    int base, n_extra;       // head: head_balanced_kernel<base, nch, f16, stamped>; n_extra = workgroups with an extra unit
    int cw, mr;              // gemv: gemv_rows_kernel<epi, ln, cw, mr>
    int nch;                 // skinny, head: k-chunks of 32 per wave (skinny: 0 = the generic instruction stream)
    bool ln, f16, stamped;   // ln: folded LayerNorm (skinny, ln_c1) or direct LayerNorm (gemv, ln_g)
    dim3 grid, block;
    int shmem;               // dynamic LDS bytes
    bool raise_lds;          // raise the kernel's dynamic-LDS limit to shmem before the launch
    int n_partials;          // LOGITS: (max, argmax) partials per row, at pmax_val / pmax_idx [row * n_partials + i]
};
// rowmajor_gemv: a.W is the row-major [N, K] matrix (with a.ln_g / a.ln_b) for the dot-product kernel; otherwise the tiled copy
int plan_decode_gemm(int epi, const SkinnyArgs& a, bool rowmajor_gemv, DecodeGemmPlan* p);
int launch_decode_gemm(int epi, const DecodeGemmPlan& p, const SkinnyArgs& a, hipStream_t st);
bool gemv_shape_ok(int M, int N, int K);   // the shapes gemv_rows_kernel takes
// a kernel's host address and its per-device "dynamic-LDS limit raised" bits (set_max_dynamic_lds): one pair per instantiation
struct KernelRef { const void* fn; uint64_t* lds_raised; };
template <auto K> KernelRef kernel_ref() {
    static uint64_t raised = 0;
    return KernelRef{reinterpret_cast<const void*>(K), &raised};
}
// the instantiation a plan names, per family (head_gemm.hip, gemv_small.hip); {nullptr, nullptr} when there is none
KernelRef head_kernel(const DecodeGemmPlan& p);
KernelRef gemv_kernel(int epi, const DecodeGemmPlan& p);
constexpr int HB_PITCH = 20;   // head_balanced_kernel: floats per LDS row of a partial tile (16 + 4: the 16 rows of one ds_write_b128
                               // start in different banks)
int launch_embed_stats(const int32_t* ids, const int32_t* lens, const int32_t* ctx_len, const float* tok_emb,
                       const float* pos_emb, float* x, float* stats, int B, int T, int C, int vocab, int pos_rows,
                       int absolute_pos, int32_t* err_flag, hipStream_t st);

}  // namespace mgea

// ---- device helpers --------------------------------------------------------------------------
#ifdef __HIPCC__
namespace mgea {
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// non-temporal 16-byte load for data streamed once (KV pages): does not displace L2/MALL lines
__device__ __forceinline__ float4 ldnt4(const float* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
// 8 floats -> 8 halves, round-to-nearest-even (v_cvt_f16_f32)
__device__ __forceinline__ h16x8 to_h8(float4 a, float4 b) {
    return (h16x8){(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w, (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
}
// the 4 consecutive elements d .. d+3 (d % 4 == 0) of head `head`, token slot `slot`, of the K (isv = 0) or V page `phys`
__device__ __forceinline__ void kv_store4(const KvPool& pool, int layer, int phys, int isv, int head, int slot, int d, float4 v) {
    const int64_t pe = pool.page_elems();
    const int64_t page = layer * pool.layer_stride + ((int64_t)(phys * 2 + isv) * pool.H + head) * pe;
    if (pool.f16) {
        _Float16* p = static_cast<_Float16*>(pool.base) + page + (isv ? slot * pool.dh + d : ((d >> 3) * MGEA_KV_PAGE_TOKENS + slot) * 8 + (d & 7));
        *reinterpret_cast<h16x4*>(p) = (h16x4){(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
    } else {
        float* p = static_cast<float*>(pool.base) + page + (isv ? slot * pool.dh + d : ((d >> 2) * MGEA_KV_PAGE_TOKENS + slot) * 4);
        st4(p, v);
    }
}

// End of a decode step for row b, by one workgroup of >= 256 threads whose thread 0 holds the new token `tok` (threads >= 256 only take part
// in the barriers; the sampler's workgroup has SAMP_NT = 256):
// the sampler-loop bookkeeping of api_cache.py:179-181 (append, EOS stop) and the NEXT step's embedding
// x[b] = tok_emb[fed] + pos_emb[pos] (k-tiled) with its LayerNorm statistics (two equal half-row partials).
// st_* = the row's state and what stops it (row_stops) as loaded by thread 0 at kernel start.  sh: >= 7 floats of shared scratch.
// With the qkv0 table (TailArgs::qkv0) the embedding goes through embed_qkv0_row instead and has no statistics.
// PENALTY: also set the token's bit in the row's presence bitmap (presence_words(vocab) words per row) while the row is not finished:
// one writer per row, read by a later kernel, so a plain read-modify-write of the word.
// The end of row b's decode step on every path (fused sampler tail, greedy argmax tails, advance_kernel), so the rule cannot drift between
// them: a row that is not finished (done = its flag at step start, len = its ctx_len then) appends tok -- ids_out, cur_ids, ctx_len + 1 --
// and finishes on its EOS id or when this was its last budgeted step (row_step + 1 == max_new): done = 1, n_done + 1.  row_step advances
// either way.  Returns the token fed to the next step; *len_out (optional) receives the row's ctx_len as the next step will read it.
// A finished row still runs every later step of its batch (fed its last token at position ctx_len, attending to ctx_len + 1 keys).  A
// row that finishes with its pages full (ctx_len = ctx_cap) would read one key past them: it is parked one position short instead --
// done = 2, ctx_len - 1, where its later steps only rewrite the last key -- and launch_unpark_rows restores both after the loop.
// (Each later step of a parked row stores the K | V of its re-fed last token at position ctx_len, over the key of the token fed before
// it: after unpark the row's ctx_len counts all its tokens, but its last cache position holds its final token, not the one before it
// as a fresh prefill of its ids would.  Nobody attends from a finished row again; a caller that continued one would have to prefill it anew.)
// Every row's NEXT position is therefore *len_out, the parked row's too: advance_embed_row embeds at it and embed_qkv0_row caches at it,
// as the unfused pair (advance_kernel, then an embedding kernel that reads ctx_len) does.  The rule is written out, and every caller
// held to it, in tests/step_tail_util.py and tests/test_gpu_step_tail.py.
// What stops row b: its record's eos_id, max_new and ctx_cap, or without records the by-value eos_id and no budget.  A caller loads
// them with the rest of the row's state (row_stops, beside row_step / cur_ids / ctx_len / done), finished rows included -- the
// record is in bounds for every row and a finished row does not use it -- so that no load stands between the new token and the
// stores that depend on it.
struct RowStops { int eos, max_new, cap; };
__device__ __forceinline__ RowStops row_stops(const mgea::StepState& s, int b) {
    RowStops r{s.eos_id, mgea::MGEA_NO_BUDGET, mgea::MGEA_NO_BUDGET};
    if (s.params) { r.eos = s.params[b].eos_id; r.max_new = s.params[b].max_new; r.cap = s.params[b].ctx_cap; }
    return r;
}
__device__ __forceinline__ int end_row_step(const mgea::StepState& s, int b, int tok, int step, int fed, int len, int done,
                                            const RowStops& stops, int* len_out = nullptr) {
    int out = -1, next_len = len;
    if (!done) {
        out = tok;
        fed = tok;
        next_len = len + 1;
        s.cur_ids[b] = tok;
        s.ctx_len[b] = len + 1;
        const int eos = stops.eos, max_new = stops.max_new, cap = stops.cap;
        if (tok == eos || step + 1 == max_new) {
            const bool park = len + 1 >= cap;
            s.done[b] = park ? 2 : 1;
            if (park) { s.ctx_len[b] = len; next_len = len; }
            atomicAdd(s.n_done, 1);
        }
    }
    if (s.ids_out && step < s.n_steps) s.ids_out[(int64_t)b * s.n_steps + step] = out;
    s.row_step[b] = step + 1;
    if (len_out) *len_out = next_len;
    return fed;
}

// The embedding of token `id` for row b with layer 0's in-projection taken from the table (TailArgs::qkv0), by threads 0..255 of a
// workgroup: x[b] = tok_emb[id] + pos_emb[pos] (k-tiled; the residual the out-projection adds to), qkv[b] = table[id] -- the whole row,
// as the EPI_QKV epilogue of gemm_skinny.hip stores it -- and its K | V part into layer 0's page at position len = the row's ctx_len as
// the next step reads it, under that epilogue's `page < max_pages` guard.  The physical page follows the decoder's allocation rule where
// the pool carries it (KvPool::arith_batch) and the page table otherwise.  Every load -- embedding rows, table row, page id -- is
// requested before the first store: one memory round trip, as the embedding alone.
// (The last step of a generation thereby stores one position the launch would not have: in bounds by the guard, beyond every row's
// length, and overwritten by whatever step comes next.)
__device__ __forceinline__ void embed_qkv0_row(int b, int id, int pos, int len, const mgea::TailArgs& t) {
    const int f = threadIdx.x, C = t.C;   // one float4 of x, q, k and v per thread: C <= 1024 (QKV0_MAX_C, checked by the launchers)
    if (f >= (C >> 2)) return;
    const int page = len >> 6, slot = len & (MGEA_KV_PAGE_TOKENS - 1);
    const bool paged = page < t.max_pages;
    int phys = 0;
    if (paged) phys = t.pool.arith_batch > 0 ? page * t.pool.arith_batch + b : t.page_table[b * t.max_pages + page];
    const float* row = t.qkv0 + (int64_t)id * 3 * C + f * 4;
    const float4 e = add4(ld4(t.tok_emb + (int64_t)id * C + f * 4), ld4(t.pos_emb + (int64_t)pos * C + f * 4));
    const float4 q = ld4(row), k = ld4(row + C), v = ld4(row + 2 * C);
    float* out = t.qkv + (int64_t)b * 3 * C + f * 4;
    st4(t.x + mgea::tiled_off(b, f * 4, C), e);
    st4(out, q);
    st4(out + C, k);
    st4(out + 2 * C, v);
    if (paged) {
        const int head = (f * 4) / t.pool.dh, d = (f * 4) % t.pool.dh;
        kv_store4(t.pool, 0, phys, 0, head, slot, d, k);
        kv_store4(t.pool, 0, phys, 1, head, slot, d, v);
    }
}

template <bool PENALTY = false>
__device__ __forceinline__ void advance_embed_row(int b, int tok, const mgea::TailArgs& t, int32_t* sampled, int st_step, int st_fed,
                                                  int st_len, int st_done, const RowStops& st_stops, float* sh,
                                                  uint32_t* presence = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* shi = reinterpret_cast<int*>(sh);
    if (tid == 0) {
        sampled[b] = tok;
        int next_len;
        const int fed = end_row_step(t.s, b, tok, st_step, st_fed, st_len, st_done, st_stops, &next_len);
        const int len = next_len;   // the position the row is fed at = its ctx_len as the next step reads it (a row parked in this step: st_len)
        shi[6] = next_len;
        if constexpr (PENALTY) {
            if (!st_done && (unsigned)tok < (unsigned)t.vocab) {
                uint32_t* w = presence + (int64_t)b * mgea::presence_words(t.vocab) + (tok >> 5);
                *w = *w | (1u << (tok & 31));
            }
        }
        shi[4] = fed < 0 ? 0 : (fed >= t.vocab ? t.vocab - 1 : fed);
        const int pos = t.absolute_pos ? len : 0;   // reference: a decode step adds pos_emb[:1] = row 0 (api_cache.py:99)
        shi[5] = pos < t.pos_rows ? pos : t.pos_rows - 1;
    }
    __syncthreads();
    const int id = shi[4], pos = shi[5];
    if (t.qkv0) {   // (a kernel argument: the whole workgroup takes this branch or none of it)
        embed_qkv0_row(b, id, pos, shi[6], t);
        return;
    }
    const int C = t.C, nf4 = C >> 2;
    float4 v[4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = tid + i * 256;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f < nf4 && tid < 256) {
            v[i] = add4(ld4(t.tok_emb + (int64_t)id * C + f * 4), ld4(t.pos_emb + (int64_t)pos * C + f * 4));
            st4(t.x + mgea::tiled_off(b, f * 4, C), v[i]);
            sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    auto bsum = [&](float val) {
        val = wave_sum(val);
        __syncthreads();
        if (lane == 0 && wave < 4) sh[wave] = val;
        __syncthreads();
        return (sh[0] + sh[1]) + (sh[2] + sh[3]);
    };
    const float mean = bsum(sum) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = tid + i * 256;
        if (f < nf4 && tid < 256) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    const float m2 = bsum(q);
    if (tid == 0) st4(t.stats + (int64_t)b * 4, make_float4(mean, 0.5f * m2, mean, 0.5f * m2));   // as embed_stats_kernel
}
}  // namespace mgea
#endif
