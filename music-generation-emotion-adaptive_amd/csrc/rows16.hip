// The row-wise kernels around the 16-bit GEMMs and attention (bf16 / fp16 in and out, fp32 statistics):
// * f32_to_bf16_kernel: fp32 -> bf16 / fp16 conversion of weights;
// * ln_rowstat_kernel, fold_ln_weights_bf16_kernel: the helpers of the folded-LayerNorm pipeline (BfEpiLn, common.h);
// * gather_cls*_kernel, layernorm_bf16_kernel, bert_embed_ln_bf16_kernel: bf16 DistilBERT;
// * dec_embed_f16_kernel, kv_scatter_f16_kernel: the fp16 prefill of the decoder.
#include "x16.h"

namespace mgea {

// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 v = ld4(src + i);
        t4 o = {(T)v.x, (T)v.y, (T)v.z, (T)v.w};
        *reinterpret_cast<t4*>(dst + i) = o;
    } else {
        for (int64_t j = i; j < n; ++j) dst[j] = (T)src[j];
    }
}
int launch_f32_to_bf16(const float* src, void* dst, int64_t n, hipStream_t st, int f16) {
    if (f16) hipLaunchKernelGGL(f32_to_bf16_kernel<_Float16>, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, st, src, (_Float16*)dst, n);
    else     hipLaunchKernelGGL(f32_to_bf16_kernel<bf16_t>, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, st, src, (bf16_t*)dst, n);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// ------------------------------------------------------------------------------------------
// Helpers of the folded-LayerNorm pipeline (BfEpiLn).
// (mean, rstd) per row from the per-tile (sum, M2 about the tile's own mean) pairs the RES_LN epilogue left, each over C / n_part
// columns: mean = sum of sums / C, M2 = sum_i M2_i + cnt sum_i (mean_i - mean)^2 (the exact pairwise merge), in double.
// A launch of its own (5 us): deriving the statistics inside the consumers instead (8-16 more loaded values live per lane in their
// epilogues) pushed 20-50 registers of the persistent kernel to scratch and cost 0.45 ms per forward.
__global__ void ln_rowstat_kernel(const float* __restrict__ part, float* __restrict__ rowstat, int M, int n_part, int C, float eps) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    const double cnt = (double)C / n_part;
    double s1 = 0.0;
    for (int i = 0; i < n_part; ++i) s1 += part[((int64_t)row * n_part + i) * 2];
    const double mean = s1 / C;
    double m2 = 0.0;
    for (int i = 0; i < n_part; ++i) {
        const double d = part[((int64_t)row * n_part + i) * 2] / cnt - mean;
        m2 += part[((int64_t)row * n_part + i) * 2 + 1] + cnt * d * d;
    }
    rowstat[(int64_t)row * 2] = (float)mean;
    rowstat[(int64_t)row * 2 + 1] = (float)(1.0 / sqrt(m2 / C + (double)eps));
}
int launch_ln_rowstat(const float* part, float* rowstat, int M, int n_part, int C, float eps, hipStream_t st) {
    hipLaunchKernelGGL(ln_rowstat_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, st, part, rowstat, M, n_part, C, eps);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// W' = bf16(W diag(gamma)), c1[n] = sum_k W'[n, k] (of the ROUNDED folded weights: the epilogue subtracts exactly what the MFMAs
// added), c2[n] = b[n] + sum_k W[n, k] beta[k].  One workgroup per output row n.
template <typename T>
__global__ __launch_bounds__(256) void fold_ln_weights_bf16_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ b,
                                                                  T* __restrict__ Wf, float* __restrict__ c1,
                                                                  float* __restrict__ c2, int K) {
    const int64_t n = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float w = W[n * K + k];
        const T wf = (T)(w * gamma[k]);
        Wf[n * K + k] = wf;
        s1 += (float)wf;
        s2 = fmaf(w, beta[k], s2);
    }
    __shared__ float r1[4], r2[4];
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = s1; r2[threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        c1[n] = (r1[0] + r1[1]) + (r1[2] + r1[3]);
        c2[n] = b[n] + ((r2[0] + r2[1]) + (r2[2] + r2[3]));
    }
}
int launch_fold_ln_weights_bf16(const float* W, const float* gamma, const float* beta, const float* b, void* Wf, float* c1, float* c2,
                                int N, int K, hipStream_t st, int f16) {
    if (f16) hipLaunchKernelGGL(fold_ln_weights_bf16_kernel<_Float16>, dim3(N), dim3(256), 0, st, W, gamma, beta, b, (_Float16*)Wf, c1, c2, K);
    else     hipLaunchKernelGGL(fold_ln_weights_bf16_kernel<bf16_t>, dim3(N), dim3(256), 0, st, W, gamma, beta, b, (bf16_t*)Wf, c1, c2, K);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// CLS rows (row b * S) of the RAW last-layer output -> LayerNorm with the row's (mean, rstd) -> fp32 [B, D]
__global__ void gather_cls_ln_bf16_kernel(const bf16_t* __restrict__ h, const float* __restrict__ rowstat, const float* __restrict__ g,
                                          const float* __restrict__ be, float* __restrict__ out, int S, int D, const int32_t* __restrict__ cu) {
    const int64_t row = cu ? (int64_t)cu[blockIdx.x] : (int64_t)blockIdx.x * S;      // the [CLS] row of sequence b (packed input: its first row)
    const float mean = rowstat[row * 2], rstd = rowstat[row * 2 + 1];
    for (int d = threadIdx.x; d < D; d += blockDim.x) out[(int64_t)blockIdx.x * D + d] = fmaf(((float)h[row * D + d] - mean) * rstd, g[d], be[d]);
}
int launch_gather_cls_ln_bf16(const void* h, const float* rowstat, const float* g, const float* be, float* out, int B, int S, int D,
                              hipStream_t st, const int32_t* cu) {
    hipLaunchKernelGGL(gather_cls_ln_bf16_kernel, dim3(B), dim3(256), 0, st, (const bf16_t*)h, rowstat, g, be, out, S, D, cu);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// ------------------------------------------------------------------------------------------
// LayerNorm over bf16 rows (fp32 statistics), in place allowed.  A wave owns 4 rows and requests all of them (and the affine
// vectors) before the first reduction: 8-16 loads of 16 bytes in flight per lane instead of 2, four independent reduction chains.
// (One row per wave ran at 4.2 TB/s of read + write on [32768, 768]: every wave sat through a load, two dependent wave reductions
// and a second round trip for w / b before its only stores.)
template <int NCHL>   // 16-byte chunks per lane and row: C <= 512 * NCHL
__global__ __launch_bounds__(256) void layernorm_bf16_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, bf16_t* __restrict__ y, int M,
                                                            int C, float eps) {
    constexpr int RW = 4;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
    if (row0 >= M) return;
    const int nch = C >> 3;  // 16-byte chunks per row
    bf16x8 t[RW][NCHL];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t row = row0 + r < M ? row0 + r : M - 1;     // clamped: loaded, never stored
#pragma unroll
        for (int i = 0; i < NCHL; ++i) {
            const int ch = lane + i * 64;
            t[r][i] = *reinterpret_cast<const bf16x8*>(x + row * C + (ch < nch ? ch : 0) * 8);
        }
    }
    float4 wv[NCHL][2], bv[NCHL][2];
#pragma unroll
    for (int i = 0; i < NCHL; ++i) {
        const int ch = lane + i * 64 < nch ? lane + i * 64 : 0;
        wv[i][0] = ld4(w + ch * 8); wv[i][1] = ld4(w + ch * 8 + 4);
        bv[i][0] = ld4(b + ch * 8); bv[i][1] = ld4(b + ch * 8 + 4);
    }
    const float inv_c = 1.0f / (float)C;
    float mean[RW], rstd[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NCHL; ++i)
            if (lane + i * 64 < nch)
#pragma unroll
                for (int j = 0; j < 8; ++j) s += (float)t[r][i][j];
        mean[r] = s;
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) mean[r] = wave_sum(mean[r]) * inv_c;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NCHL; ++i)
            if (lane + i * 64 < nch)
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = (float)t[r][i][j] - mean[r]; q += d * d; }
        rstd[r] = q;
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) rstd[r] = 1.0f / sqrtf(wave_sum(rstd[r]) * inv_c + eps);
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        if (row0 + r >= M) break;
#pragma unroll
        for (int i = 0; i < NCHL; ++i) {
            const int ch = lane + i * 64;
            if (ch < nch) {
                const float ww[8] = {wv[i][0].x, wv[i][0].y, wv[i][0].z, wv[i][0].w, wv[i][1].x, wv[i][1].y, wv[i][1].z, wv[i][1].w};
                const float bb[8] = {bv[i][0].x, bv[i][0].y, bv[i][0].z, bv[i][0].w, bv[i][1].x, bv[i][1].y, bv[i][1].z, bv[i][1].w};
                bf16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(((float)t[r][i][j] - mean[r]) * rstd[r] * ww[j] + bb[j]);
                *reinterpret_cast<bf16x8*>(y + (row0 + r) * C + ch * 8) = o;
            }
        }
    }
}
int launch_layernorm_bf16(const void* x, const float* w, const float* b, void* y, int M, int C, float eps, hipStream_t st) {
    MGEA_REQUIRE(C % 8 == 0 && C <= 2048, MGEA_EINVAL, "bf16 layernorm: C=%d must be a multiple of 8 and <= 2048", C);
    const dim3 grid(ceil_div(M, 16));
    if (C <= 1024) hipLaunchKernelGGL(layernorm_bf16_kernel<2>, grid, dim3(256), 0, st, (const bf16_t*)x, w, b, (bf16_t*)y, M, C, eps);
    else           hipLaunchKernelGGL(layernorm_bf16_kernel<4>, grid, dim3(256), 0, st, (const bf16_t*)x, w, b, (bf16_t*)y, M, C, eps);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// h[m] = LN(word[ids[m]] + pos[t]) -> bf16 (fp32 tables)
__global__ __launch_bounds__(256) void bert_embed_ln_bf16_kernel(const int32_t* __restrict__ ids, const float* __restrict__ word,
                                                                const float* __restrict__ pos, const float* __restrict__ lnw,
                                                                const float* __restrict__ lnb, float eps,
                                                                bf16_t* __restrict__ h, int M, int S, int D, int vocab,
                                                                int32_t* __restrict__ err_flag, const int32_t* __restrict__ pos_ids) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int t = pos_ids ? pos_ids[row] : (int)(row % S);      // packed input carries each row's position in its sequence
    int id = ids[row];
    if ((id < 0 || id >= vocab) && err_flag && lane == 0) atomicOr(err_flag, 1);   // clamped + reported (mgea_bert_error_flags)
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int nf4 = D >> 2;
    float4 v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + i * 64;
        if (f < nf4) {
            v[i] = add4(ld4(word + (int64_t)id * D + f * 4), ld4(pos + (int64_t)t * D + f * 4));
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (lane + i * 64 < nf4) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + i * 64;
        if (f < nf4) {
            const float4 ww = ld4(lnw + f * 4), bb = ld4(lnb + f * 4);
            bf16x4 o = {(bf16_t)((v[i].x - mean) * rstd * ww.x + bb.x), (bf16_t)((v[i].y - mean) * rstd * ww.y + bb.y),
                        (bf16_t)((v[i].z - mean) * rstd * ww.z + bb.z), (bf16_t)((v[i].w - mean) * rstd * ww.w + bb.w)};
            *reinterpret_cast<bf16x4*>(h + row * D + f * 4) = o;
        }
    }
}
int launch_bert_embed_ln_bf16(const int32_t* ids, const float* word, const float* pos, const float* lnw, const float* lnb,
                              float eps, void* h, int B, int S, int D, int vocab, hipStream_t st, int32_t* err_flag, const int32_t* pos_ids) {
    MGEA_REQUIRE(D % 4 == 0 && D <= 2048, MGEA_EINVAL, "bf16 embed: dim=%d must be a multiple of 4 and <= 2048", D);
    // (packed input: B = the number of rows, S = 1)
    hipLaunchKernelGGL(bert_embed_ln_bf16_kernel, dim3(ceil_div(B * S, 4)), dim3(256), 0, st, ids, word, pos, lnw, lnb, eps,
                       (bf16_t*)h, B * S, S, D, vocab, err_flag, pos_ids);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// CLS rows (row b*S) of a bf16 [B*S, D] matrix -> fp32 [B, D] for the small fp32 classifier head
__global__ void gather_cls_bf16_kernel(const bf16_t* __restrict__ h, float* __restrict__ out, int S, int D, const int32_t* __restrict__ cu) {
    const int64_t b = blockIdx.x, row = cu ? (int64_t)cu[b] : b * S;
    for (int d = threadIdx.x; d < D; d += blockDim.x) out[b * D + d] = (float)h[row * D + d];
}
int launch_gather_cls_bf16(const void* h, float* out, int B, int S, int D, hipStream_t st, const int32_t* cu) {
    hipLaunchKernelGGL(gather_cls_bf16_kernel, dim3(B), dim3(256), 0, st, (const bf16_t*)h, out, S, D, cu);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// ------------------------------------------------------------------------------------------
// fp16 big-batch prefill of the decoder (MGEA_DTYPE_F16, decoder.hip: run_prefill16): the pre-LN GPT block on the GEMM and attention kernels of gemm16.hip / attn16.hip with
// _Float16 operands.  Three small kernels around them:
// x[m] = f16(tok_emb[ids[m]] + pos_emb[pos]) and the (mean, rstd) of the ROUNDED row (what the folded-LayerNorm GEMM consumes);
// rows with t >= lens[b] are zero rows with the identity statistics (0, 1).  One wave per row.
__global__ __launch_bounds__(256) void dec_embed_f16_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens,
                                                           const int32_t* __restrict__ ctx_len, const float* __restrict__ tok_emb,
                                                           const float* __restrict__ pos_emb, _Float16* __restrict__ x,
                                                           float* __restrict__ rowstat, int32_t* __restrict__ mask_out, float eps, int M,
                                                           int T, int C, int vocab, int pos_rows, int absolute_pos,
                                                           int32_t* __restrict__ err_flag) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int b = (int)(m / T), t = (int)(m % T);
    const bool real = lens ? (t < lens[b]) : true;
    int id = ids[m];
    if (real && (id < 0 || id >= vocab) && err_flag && lane == 0) atomicOr(err_flag, 1);
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pos = t + ((absolute_pos && ctx_len) ? ctx_len[b] : 0);
    pos = pos < pos_rows ? pos : pos_rows - 1;
    const int nf4 = C >> 2;
    float4 v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = lane + i * 64;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f < nf4 && real) {
            const float4 e = add4(ld4(tok_emb + (int64_t)id * C + f * 4), ld4(pos_emb + (int64_t)pos * C + f * 4));
            const h16x4 o = {(_Float16)e.x, (_Float16)e.y, (_Float16)e.z, (_Float16)e.w};
            v[i] = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
        }
        if (f < nf4) {
            const h16x4 o = {(_Float16)v[i].x, (_Float16)v[i].y, (_Float16)v[i].z, (_Float16)v[i].w};
            *reinterpret_cast<h16x4*>(x + m * C + f * 4) = o;
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (lane + i * 64 < nf4) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    const float var = wave_sum(q) / (float)C;
    if (lane == 0) {
        *reinterpret_cast<float2*>(rowstat + m * 2) = real ? make_float2(mean, 1.0f / sqrtf(var + eps)) : make_float2(0.f, 1.f);
        if (mask_out) mask_out[m] = real ? 1 : 0;           // the key validity the dense attention wants for ragged prompts
    }
}
int launch_dec_embed_f16(const int32_t* ids, const int32_t* lens, const int32_t* ctx_len, const float* tok_emb, const float* pos_emb,
                         void* x, float* rowstat, int32_t* mask_out, float eps, int B, int T, int C, int vocab, int pos_rows, int absolute_pos,
                         int32_t* err_flag, hipStream_t st) {
    MGEA_REQUIRE(C % 4 == 0 && C <= 2048, MGEA_EINVAL, "fp16 embed: d_model=%d must be a multiple of 4 and <= 2048", C);
    hipLaunchKernelGGL(dec_embed_f16_kernel, dim3(ceil_div(B * T, 4)), dim3(256), 0, st, ids, lens, ctx_len, tok_emb, pos_emb,
                       (_Float16*)x, rowstat, mask_out, eps, B * T, T, C, vocab, pos_rows, absolute_pos, err_flag);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

// K | V columns of the fp16 qkv rows [M, 3C] -> the fp16 KV pages of `layer` (common.h: K [dh/8][64 tokens][8], V [64 tokens][dh]):
// one thread per 16-byte group, real tokens only, position ctx_len[b] + t.
__global__ __launch_bounds__(256) void kv_scatter_f16_kernel(const _Float16* __restrict__ qkv, KvPool pool, int layer,
                                                            const int32_t* __restrict__ page_table, int max_pages,
                                                            const int32_t* __restrict__ ctx_len, const int32_t* __restrict__ lens,
                                                            int64_t n_groups, int T, int C) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n_groups) return;
    const int gpr = (2 * C) >> 3;                       // 16-byte groups of K | V per row
    const int64_t m = gid / gpr;
    const int gi = (int)(gid - m * gpr);
    const int b = (int)(m / T), t = (int)(m % T);
    const bool real = lens ? (t < lens[b]) : true;
    if (!real) return;
    const int pos = ctx_len[b] + t;
    const int page = pos >> 6, slot = pos & 63;
    if (page >= max_pages) return;
    const int phys = page_table[b * max_pages + page];
    const int n = gi * 8;                                // column inside K | V
    const int isv = n >= C, nn = n - (isv ? C : 0), head = nn / pool.dh, d = nn % pool.dh;
    const float4 raw = *reinterpret_cast<const float4*>(qkv + m * 3 * C + C + n);
    const int64_t pe = pool.page_elems();
    _Float16* pg = static_cast<_Float16*>(pool.base) + layer * pool.layer_stride + ((int64_t)(phys * 2 + isv) * pool.H + head) * pe;
    *reinterpret_cast<float4*>(pg + (isv ? slot * pool.dh + d : ((d >> 3) * MGEA_KV_PAGE_TOKENS + slot) * 8)) = raw;
}
int launch_kv_scatter_f16(const void* qkv, const KvPool& pool, int layer, const int32_t* page_table, int max_pages, const int32_t* ctx_len,
                          const int32_t* lens, int B, int T, int C, hipStream_t st) {
    MGEA_REQUIRE(pool.f16 && pool.dh % 8 == 0 && C % 8 == 0, MGEA_EINVAL, "fp16 KV scatter needs fp16 pages and head_dim %% 8 == 0");
    const int64_t n_groups = (int64_t)B * T * ((2 * C) >> 3);
    hipLaunchKernelGGL(kv_scatter_f16_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, (const _Float16*)qkv, pool, layer,
                       page_table, max_pages, ctx_len, lens, n_groups, T, C);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
