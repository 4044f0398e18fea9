// Classifier-free guidance between paired rows of a logits matrix [B, V] (include/mgea.h, mgea_decoder_generate_rows_guided): the
// launch between the head GEMM and the sampler of a guided decode step.  A conditional row c and its shadow row u = partner[c] -- the
// same generation from a prompt without the conditioning tokens -- are combined in log-probability space,
//   g = s * log_softmax(x_c) + (1 - s) * log_softmax(x_u),   s = scale[c],
// and g is written into BOTH rows: the two sampler workgroups behind this launch then compute the same function of the same row (the
// engine has made the rest of their inputs equal), so both rows take the same id without any hand-off between workgroups.
// HuggingFace's counterpart is UnbatchedClassifierFreeGuidanceLogitsProcessor (guidance_scale); it comes first there too, before the
// repetition penalty.
#include "common.h"

namespace mgea {

constexpr int GUIDE_NT = 256, GUIDE_NW = GUIDE_NT / 64;   // threads / waves per row: the sampler's geometry

// One GUIDE_NT-thread workgroup per batch row; workgroup c does the pair (c, partner[c]), every other workgroup returns at once -- the
// grid, and with it the captured step graph, does not depend on which rows are paired.  partner[b] is the row's own word, so the exit
// is block-uniform.  Nobody else touches the two rows: a shadow is never conditional itself and never shadows two rows (checked on
// the host), so its own workgroup is one of those that return.
// As in sample_kernel thread t owns the ids t, t + 256, ... of both rows in registers (MAXE each, padding -inf), requested in ONE
// batch of loads; the rows go to memory once and never through LDS.  The maximum and the exp-sum of each row are reduced in a fixed
// order -- per thread ascending j, a butterfly inside the wave, the four wave values left to right through LDS -- in fp32, without
// atomics: the result is the same bits from run to run.  Inputs are finite (the head GEMM of finite weights), so m is finite, the
// sum is >= 1 and g is finite for a finite scale.
template <int MAXE>
__global__ __launch_bounds__(GUIDE_NT) void guidance_mix_kernel(float* __restrict__ logits, int B, int V,
                                                                const int32_t* __restrict__ partner, const float* __restrict__ scale) {
    constexpr int NT = GUIDE_NT, NW = GUIDE_NW;
    static_assert(NW == 4, "the merges below name four wave values");
    const int c = blockIdx.x, tid = threadIdx.x;
    const int u = partner[c];
    if (u < 0 || u >= B) return;   // (>= B: the hosts check their pairs; a stray word must not reach memory)
    const float s = scale[c];
    float* rc = logits + (int64_t)c * V;
    float* ru = logits + (int64_t)u * V;
    float xc[MAXE], xu[MAXE];
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const int i = tid + NT * j;
        xc[j] = i < V ? rc[i] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const int i = tid + NT * j;
        xu[j] = i < V ? ru[i] : -INFINITY;
    }
    __shared__ float s_max[2][NW], s_sum[2][NW];
    float mc = -INFINITY, mu = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        mc = fmaxf(mc, xc[j]);
        mu = fmaxf(mu, xu[j]);
    }
    mc = wave_max(mc);
    mu = wave_max(mu);
    if ((tid & 63) == 0) {
        s_max[0][tid >> 6] = mc;
        s_max[1][tid >> 6] = mu;
    }
    __syncthreads();
    mc = fmaxf(fmaxf(s_max[0][0], s_max[0][1]), fmaxf(s_max[0][2], s_max[0][3]));
    mu = fmaxf(fmaxf(s_max[1][0], s_max[1][1]), fmaxf(s_max[1][2], s_max[1][3]));
    float ec = 0.f, eu = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        ec += __expf(xc[j] - mc);   // the padding beyond V is -inf: exactly 0
        eu += __expf(xu[j] - mu);
    }
    ec = wave_sum(ec);
    eu = wave_sum(eu);
    if ((tid & 63) == 0) {
        s_sum[0][tid >> 6] = ec;
        s_sum[1][tid >> 6] = eu;
    }
    __syncthreads();
    const float lc = logf((s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]));
    const float lu = logf((s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]));
    const float t = 1.f - s;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const int i = tid + NT * j;
        if (i < V) {
            const float g = s * (xc[j] - mc - lc) + t * (xu[j] - mu - lu);
            rc[i] = g;
            ru[i] = g;
        }
    }
}

int launch_guidance_mix(float* logits, int B, int V, const int32_t* partner, const float* scale, hipStream_t st) {
    MGEA_REQUIRE(logits && partner && scale && B > 0, MGEA_EINVAL, "guidance mix: NULL argument or empty batch");
    MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "guidance mix: vocab %d exceeds the register-resident row (%d)", V,
                 MGEA_SAMPLER_MAX_VOCAB);
    static_assert(GUIDE_NT * 56 >= MGEA_SAMPLER_MAX_VOCAB, "the register-resident rows must hold the largest vocabulary");
    auto kern = V <= GUIDE_NT * 36 ? guidance_mix_kernel<36> : guidance_mix_kernel<56>;
    hipLaunchKernelGGL(kern, dim3(B), dim3(GUIDE_NT), 0, st, logits, B, V, partner, scale);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
