// The end of a decode step, after the LM head: the greedy argmax tails, the bookkeeping kernel behind an unfused sampler launch, the
// presence bitmaps' seed, the grammar's allow bitmask, and the rows' sampler records (their host checks, the builder, the kernels that fill and clamp them).
// The sampler itself is sampler.hip; end_row_step / advance_embed_row, which every tail shares, are in common.h.
#include <cmath>

#include "common.h"

namespace mgea {

// ------------------------------------------------------------------------------------------
// greedy finalize: argmax over the per-tile partials of each row, then the sampler-loop
// bookkeeping of api_cache.py:179-181 (append, EOS or budget stop: end_row_step) -- one 64-thread workgroup per row.
__global__ __launch_bounds__(64) void argmax_advance_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                           int n_tiles, StepState s, int32_t* __restrict__ sampled) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < n_tiles; i += 64) {
        const float v = pval[(int64_t)b * n_tiles + i];
        const int ix = pidx[(int64_t)b * n_tiles + i];
        if (v > best || (v == best && ix < bi)) { best = v; bi = ix; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        const int tok = bi == 0x7fffffff ? 0 : bi;
        sampled[b] = tok;
        end_row_step(s, b, tok, s.row_step[b], s.cur_ids[b], s.ctx_len[b], s.done[b], row_stops(s, b));
    }
}

// Same finalize fused with the NEXT step's embedding (generate() keeps x "primed"): one launch less
// per decode step.  256 threads per row: partial-argmax reduce, bookkeeping by thread 0, then
// x[row] = tok_emb[token] + pos_emb[pos] (k-tiled) and its LayerNorm partial statistics.
__global__ __launch_bounds__(256) void argmax_advance_embed_kernel(const float* __restrict__ pval,
                                                                  const int32_t* __restrict__ pidx, int n_tiles,
                                                                  TailArgs t, int32_t* __restrict__ sampled) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float sh[8];
    // The argument block in ONE batch of scalar loads and one wait: the row index below is "computed from" every field (two empty
    // statements, 30 operands each at most), so all of them are fetched in front of the first address that needs one -- the compiler
    // otherwise fetches them where they are first used, in four batches with a wait each (tools/prologue_chain.py).
    int zero;
    asm("s_mov_b32 %0, 0" : "=s"(zero) : "s"(pval), "s"(pidx), "s"(n_tiles), "s"(sampled), "s"(t.s.cur_ids), "s"(t.s.ctx_len), "s"(t.s.done),
        "s"(t.s.row_step), "s"(t.s.n_done), "s"(t.s.ids_out), "s"(t.s.n_steps), "s"(t.s.eos_id), "s"(t.s.params), "s"(t.tok_emb), "s"(t.pos_emb),
        "s"(t.x), "s"(t.stats), "s"(t.C), "s"(t.vocab), "s"(t.pos_rows), "s"(t.absolute_pos));
    asm("" : "+s"(zero) : "s"(t.qkv0), "s"(t.qkv), "s"(t.pool.base), "s"(t.pool.n_pages), "s"(t.pool.H), "s"(t.pool.dh), "s"(t.pool.spare),
        "s"(t.pool.layer_stride),
        "s"(t.pool.f16), "s"(t.pool.arith_batch), "s"(t.page_table), "s"(t.max_pages));
    const int b = blockIdx.x + zero, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the row's bookkeeping state is requested together with the partials (one round trip instead of two): four scalar loads by every
    // wave -- only thread 0 uses them, but loaded by it alone they were awaited, as that thread's values, in front of the partials' loads
    // -- and with them what stops the row (its record's eos_id, max_new and ctx_cap: finished rows load them too, in bounds and unused):
    // loaded behind the argmax they were one more dependent round trip in front of the barrier that releases the gather
    const int st_step = t.s.row_step[b], st_fed = t.s.cur_ids[b], st_len = t.s.ctx_len[b], st_done = t.s.done[b];
    const RowStops st_stops = row_stops(t.s, b);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < n_tiles; i += 256) {
        const float v = pval[(int64_t)b * n_tiles + i];
        const int ix = pidx[(int64_t)b * n_tiles + i];
        if (v > best || (v == best && ix < bi)) { best = v; bi = ix; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { sv[wave] = best; si[wave] = bi; }
    __syncthreads();
    int tok = 0;
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        tok = bi == 0x7fffffff ? 0 : bi;
    }
    advance_embed_row(b, tok, t, sampled, st_step, st_fed, st_len, st_done, st_stops, sh);
}

int launch_argmax_advance_embed(const float* pval, const int32_t* pidx, int n_tiles, const TailArgs& t, int32_t* sampled, int B,
                                hipStream_t st) {
    MGEA_REQUIRE(B <= MGEA_FUSED_MAX_ROWS && t.C % 4 == 0 && t.C <= 4096 && tail_qkv0_ok(t), MGEA_EINVAL, "argmax+embed: bad shape");
    hipLaunchKernelGGL(argmax_advance_embed_kernel, dim3(B), dim3(256), 0, st, pval, pidx, n_tiles, t, sampled);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// The embedding of ids[b] through the qkv0 table, for a row whose step is not the tail of another: generate()'s re-fed last prompt token.
__global__ __launch_bounds__(256) void embed_qkv0_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ ctx_len, TailArgs t,
                                                        int32_t* __restrict__ err_flag) {
    const int b = blockIdx.x;
    int id = ids[b];
    if ((id < 0 || id >= t.vocab) && err_flag && threadIdx.x == 0) atomicOr(err_flag, 1);   // as embed_stats_kernel
    id = id < 0 ? 0 : (id >= t.vocab ? t.vocab - 1 : id);
    const int len = ctx_len[b];
    int pos = t.absolute_pos ? len : 0;
    pos = pos < t.pos_rows ? pos : t.pos_rows - 1;
    embed_qkv0_row(b, id, pos, len, t);
}

int launch_embed_qkv0(const int32_t* ids, const int32_t* ctx_len, const TailArgs& t, int B, int32_t* err_flag, hipStream_t st) {
    MGEA_REQUIRE(t.qkv0 && tail_qkv0_ok(t) && B <= MGEA_FUSED_MAX_ROWS, MGEA_EINVAL, "embed (qkv0 table): no table, fp16 KV pages or a bad shape");
    hipLaunchKernelGGL(embed_qkv0_kernel, dim3(B), dim3(256), 0, st, ids, ctx_len, t, err_flag);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

int launch_argmax_advance(const float* pval, const int32_t* pidx, int n_tiles, const StepState& s, int32_t* sampled,
                          int B, hipStream_t st) {
    hipLaunchKernelGGL(argmax_advance_kernel, dim3(B), dim3(64), 0, st, pval, pidx, n_tiles, s, sampled);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// ------------------------------------------------------------------------------------------
// PENALTY: a row that is not finished also sets its token's bit in its presence bitmap (one thread per row: a plain read-modify-write)
template <bool PENALTY>
__device__ __forceinline__ void advance_row(int b, const int32_t* __restrict__ sampled, const StepState& s, uint32_t* __restrict__ presence,
                                            int V, int* step_out, int* done_out) {
    const int done = s.done[b], tok = sampled[b], step = s.row_step[b];
    end_row_step(s, b, tok, step, s.cur_ids[b], s.ctx_len[b], done, row_stops(s, b));   // ctx_len + 1: the token fed this step now sits in the cache
    if constexpr (PENALTY) {
        if (!done && (unsigned)tok < (unsigned)V) {
            uint32_t* w = presence + (int64_t)b * presence_words(V) + (tok >> 5);
            *w = *w | (1u << (tok & 31));
        }
    }
    *step_out = step;
    *done_out = done;
}

template <bool PENALTY>
__global__ void advance_kernel(const int32_t* __restrict__ sampled, StepState s, int B, uint32_t* __restrict__ presence, int V) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int step, done;
    advance_row<PENALTY>(b, sampled, s, presence, V, &step, &done);
}

// the same behind a scored sampler launch: the step's two log-probabilities go to the histories at the row's step, 0 for a row that was
// already finished (as the fused tail files them)
template <bool PENALTY>
__global__ void advance_scored_kernel(const int32_t* __restrict__ sampled, StepState s, int B, uint32_t* __restrict__ presence, int V,
                                      ScoreFile f) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int step, done;
    advance_row<PENALTY>(b, sampled, s, presence, V, &step, &done);
    if (step < f.stride) {
        f.logprob_hist[(int64_t)b * f.stride + step] = done ? 0.f : f.logprob_step[b];
        f.choice_hist[(int64_t)b * f.stride + step] = done ? 0.f : f.choice_step[b];
    }
}

int launch_advance(const int32_t* sampled, const StepState& s, int B, hipStream_t st, uint32_t* presence, int V, const ScoreFile* score) {
    if (score) {
        hipLaunchKernelGGL(presence ? advance_scored_kernel<true> : advance_scored_kernel<false>, dim3(ceil_div(B, 256)), dim3(256), 0, st,
                           sampled, s, B, presence, V, *score);
        MGEA_CHECK_HIP(hipGetLastError());
        return MGEA_OK;
    }
    hipLaunchKernelGGL(presence ? advance_kernel<true> : advance_kernel<false>, dim3(ceil_div(B, 256)), dim3(256), 0, st, sampled, s, B,
                       presence, V);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// One workgroup per row: the row's bitmap is built in LDS (the prompt may repeat ids, so its bits are OR-ed there), then stored whole --
// which also clears whatever an earlier generation left in it.
constexpr int PRESENCE_MAX_WORDS = (MGEA_SAMPLER_MAX_VOCAB + 31) / 32;
__global__ __launch_bounds__(256) void presence_seed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, int T, int V,
                                                            uint32_t* __restrict__ presence) {
    __shared__ uint32_t bits[PRESENCE_MAX_WORDS];
    const int b = blockIdx.x, nw = presence_words(V);
    for (int w = threadIdx.x; w < nw; w += blockDim.x) bits[w] = 0u;
    __syncthreads();
    int n = lens ? lens[b] : T;
    n = n < 0 ? 0 : (n > T ? T : n);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int id = ids[(int64_t)b * T + t];
        if ((unsigned)id < (unsigned)V) atomicOr(&bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    for (int w = threadIdx.x; w < nw; w += blockDim.x) presence[(int64_t)b * nw + w] = bits[w];
}

int launch_presence_seed(const int32_t* ids, const int32_t* lens, int B, int T, int V, uint32_t* presence, hipStream_t st) {
    MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "presence: vocab %d exceeds %d", V, MGEA_SAMPLER_MAX_VOCAB);
    hipLaunchKernelGGL(presence_seed_kernel, dim3(B), dim3(256), 0, st, ids, lens, T, V, presence);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// params_dev[0, B) <- v with stream = b, stream-ordered (a kernel argument, so no host buffer has to outlive the call)
__global__ void fill_sampler_params_kernel(SamplerParams* __restrict__ dst, SamplerParams v, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    v.stream = (uint32_t)b;
    dst[b] = v;
}

int launch_fill_sampler_params(SamplerParams* params_dev, const SamplerParams& v, int B, hipStream_t st) {
    hipLaunchKernelGGL(fill_sampler_params_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, params_dev, v, B);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

__global__ void clamp_budgets_kernel(SamplerParams* __restrict__ p, const int32_t* __restrict__ lens, int T, int B, int reserved) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = lens ? lens[b] : T;
    n = n < 1 ? 1 : (n > T ? T : n);
    const int room = reserved - n;   // >= 1: the caller checked T < reserved
    if (p[b].max_new > room) p[b].max_new = room;
    p[b].ctx_cap = reserved;
}

int launch_clamp_budgets(SamplerParams* params_dev, const int32_t* lens, int T, int B, int reserved, hipStream_t st) {
    MGEA_REQUIRE(T < reserved, MGEA_EINVAL, "budgets: prompt width %d leaves no room in %d tokens", T, reserved);
    hipLaunchKernelGGL(clamp_budgets_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, params_dev, lens, T, B, reserved);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

__global__ void unpark_rows_kernel(int32_t* __restrict__ done, int32_t* __restrict__ ctx_len, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && done[b] == 2) {
        done[b] = 1;
        ctx_len[b] += 1;
    }
}

int launch_unpark_rows(int32_t* done, int32_t* ctx_len, int B, hipStream_t st) {
    hipLaunchKernelGGL(unpark_rows_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, st, done, ctx_len, B);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// One thread per word of the allow bitmask: bit c & 31 of allow[s][c >> 5] = next[s][c] >= 0
__global__ void grammar_allow_kernel(const int32_t* __restrict__ next, int n_state, int n_class, int words, uint32_t* __restrict__ allow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_state * words) return;
    const int s = i / words, w = i - s * words;
    uint32_t bits = 0u;
    for (int k = 0; k < 32; ++k) {
        const int c = w * 32 + k;
        if (c < n_class && next[(int64_t)s * n_class + c] >= 0) bits |= 1u << k;
    }
    allow[i] = bits;
}

int launch_grammar_allow(const int32_t* next, int n_state, int n_class, uint32_t* allow, hipStream_t st) {
    MGEA_REQUIRE(n_state > 0 && n_state <= MGEA_GRAMMAR_MAX_STATES && n_class > 0 && n_class <= MGEA_GRAMMAR_MAX_CLASSES &&
                     (int64_t)n_state * n_class <= MGEA_GRAMMAR_MAX_CELLS,
                 MGEA_EINVAL, "grammar: %d states x %d classes exceed the caps", n_state, n_class);
    const int words = grammar_words(n_class);
    hipLaunchKernelGGL(grammar_allow_kernel, dim3(ceil_div(n_state * words, 256)), dim3(256), 0, st, next, n_state, n_class, words, allow);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

RowRecords build_row_records(const mgea_row_sampler* rows, const mgea_row_logits* lrows, int B, int n_steps, SamplerParams* out) {
    for (int b = 0; b < B; ++b) {
        out[b] = sampler_params(rows[b]);
        if (!lrows) continue;
        out[b].bias_on = lrows[b].bias_dev ? 1 : 0;
        out[b].min_new = lrows[b].min_new_tokens;
    }
    return row_records(rows, lrows, B, n_steps);
}

}  // namespace mgea
