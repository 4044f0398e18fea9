// Emotion blends: weighted groups of rows of a logits matrix [B, V] mixed in log-probability space (include/mgea.h,
// mgea_decoder_generate_rows_blended): the launch between the head GEMM and the sampler of a blended decode step, the N-row form of the
// guidance mix (guidance.hip).  A group is the rows b with leader[b] == L, its members m_0 < m_1 < ... < m_{K-1} in ascending row index
// (the leader L wherever it falls), and
//   g = w_0 * log_softmax(x_{m_0}),  g += w_k * log_softmax(x_{m_k})  for k = 1 .. K-1,   w_k = weight[m_k],
// goes into ALL K rows: the K sampler workgroups behind this launch then compute the same function of the same row (the engine has
// made the rest of their inputs equal), so every member takes its leader's id without any hand-off between workgroups.
#include "common.h"

namespace mgea {

constexpr int BLEND_NT = 256, BLEND_NW = BLEND_NT / 64;   // threads / waves per row: the sampler's geometry

// One BLEND_NT-thread workgroup per batch row; workgroup b does the group it leads (leader[b] == b), every other workgroup returns at
// once -- the grid, and with it the captured step graph, does not depend on the groups.  leader[b] is the row's own word, so the exit
// is block-uniform.  Nobody else touches the group's rows: a member names one leader, and its own workgroup is one of those that return.
// The first wave finds the members: 64 rows at a time each lane compares one word of the leader vector, a ballot gives every hit its
// place in ascending order, and the row indices and weights go to LDS -- indices come from the scan over [0, B) alone, so none outside
// it reaches memory; hits beyond MGEA_BLEND_MAX_ROWS (the hosts refuse such a group) are dropped.
// The members are then walked one at a time.  As in guidance_mix_kernel thread t owns the ids t, t + 256, ... of the row in registers
// (MAXE, padding -inf), read once and never through LDS; the row's maximum and exp-sum are reduced in that kernel's order -- per thread
// ascending j, a butterfly inside the wave, the four wave values left to right through LDS -- in fp32, without atomics, and w_k a_k
// is accumulated into a second register row.  g is written once to each of the K rows: the same bits from run to run.  Inputs are
// finite (the head GEMM of finite weights), so every m is finite, every sum is >= 1 and g is finite for finite weights.
template <int MAXE>
__global__ __launch_bounds__(BLEND_NT) void blend_mix_kernel(float* __restrict__ logits, int B, int V, const int32_t* __restrict__ leader,
                                                             const float* __restrict__ weight) {
    constexpr int NT = BLEND_NT, NW = BLEND_NW;
    static_assert(NW == 4, "the merges below name four wave values");
    const int b = blockIdx.x, tid = threadIdx.x;
    if (leader[b] != b) return;
    __shared__ int s_row[MGEA_BLEND_MAX_ROWS];
    __shared__ float s_w[MGEA_BLEND_MAX_ROWS];
    __shared__ int s_n;
    __shared__ float s_max[NW], s_sum[NW];
    if (tid < 64) {
        int n = 0;
        for (int base = 0; base < B; base += 64) {
            const int i = base + tid;
            const bool hit = i < B && leader[i] == b;
            const unsigned long long mask = __ballot(hit);
            if (hit) {
                const int pos = n + __popcll(mask & ((1ull << tid) - 1ull));
                if (pos < MGEA_BLEND_MAX_ROWS) {
                    s_row[pos] = i;
                    s_w[pos] = weight[i];
                }
            }
            n += __popcll(mask);
        }
        if (tid == 0) s_n = n < MGEA_BLEND_MAX_ROWS ? n : MGEA_BLEND_MAX_ROWS;
    }
    __syncthreads();
    const int K = s_n;
    float x[MAXE], g[MAXE];
    for (int k = 0; k < K; ++k) {
        const float* r = logits + (int64_t)s_row[k] * V;
        const float w = s_w[k];
#pragma unroll
        for (int j = 0; j < MAXE; ++j) {
            const int i = tid + NT * j;
            x[j] = i < V ? r[i] : -INFINITY;
        }
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < MAXE; ++j) m = fmaxf(m, x[j]);
        m = wave_max(m);
        if ((tid & 63) == 0) s_max[tid >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < MAXE; ++j) e += __expf(x[j] - m);   // the padding beyond V is -inf: exactly 0
        e = wave_sum(e);
        if ((tid & 63) == 0) s_sum[tid >> 6] = e;
        __syncthreads();   // (the next member's s_max is written behind this barrier, its s_sum behind the next one)
        const float l = logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
        if (k == 0) {
#pragma unroll
            for (int j = 0; j < MAXE; ++j) g[j] = w * (x[j] - m - l);
        } else {
#pragma unroll
            for (int j = 0; j < MAXE; ++j) g[j] += w * (x[j] - m - l);
        }
    }
    for (int k = 0; k < K; ++k) {
        float* r = logits + (int64_t)s_row[k] * V;
#pragma unroll
        for (int j = 0; j < MAXE; ++j) {
            const int i = tid + NT * j;
            if (i < V) r[i] = g[j];
        }
    }
}

int launch_blend_mix(float* logits, int B, int V, const int32_t* leader, const float* weight, hipStream_t st) {
    MGEA_REQUIRE(logits && leader && weight && B > 0, MGEA_EINVAL, "blend mix: NULL argument or empty batch");
    MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "blend mix: vocab %d exceeds the register-resident row (%d)", V,
                 MGEA_SAMPLER_MAX_VOCAB);
    static_assert(BLEND_NT * 56 >= MGEA_SAMPLER_MAX_VOCAB, "the register-resident rows must hold the largest vocabulary");
    auto kern = V <= BLEND_NT * 36 ? blend_mix_kernel<36> : blend_mix_kernel<56>;
    hipLaunchKernelGGL(kern, dim3(B), dim3(BLEND_NT), 0, st, logits, B, V, leader, weight);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
