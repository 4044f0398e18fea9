// Log-probabilities of given tokens from a matrix of logits: out[m] = logits[m][targets[m]] - logsumexp(logits[m]).
// What DecoderEngine.score_prefill gathers from the logits of ONE causal prefill (position t scores token t + 1), where a step-by-step
// scoring runs one decode step per token.
//
// One 256-thread workgroup per row, two passes over it (the second one is served by the caches: a row is at most 56 KiB): the maximum,
// then the sum of exp(x - max).  The row is read with 16-byte loads over its 16-byte-aligned middle; the up to three entries in front
// of and behind it are read one by one.  Every entry belongs to a fixed thread, every thread reduces in index order, the waves by the
// xor tree and the four wave results in wave order: the result does not depend on timing.
// targets[m] < 0: the row is not scored, out[m] = 0.  targets[m] >= V reads entry V - 1 (the host wrapper refuses it where it can see
// the ids).  A row whose entries are all -inf has no distribution: NaN, as log_softmax gives.
#include "common.h"

namespace mgea {

__global__ __launch_bounds__(256) void logprob_gather_kernel(const float* __restrict__ logits, int64_t ld,
                                                            const int32_t* __restrict__ targets, float* __restrict__ out, int V) {
    __shared__ float s_red[4];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int tgt = targets[m];
    if (tgt < 0) {   // (uniform over the workgroup)
        if (tid == 0) out[m] = 0.f;
        return;
    }
    tgt = tgt < V ? tgt : V - 1;
    const float* row = logits + m * ld;
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3);   // entries in front of the first 16-byte boundary
    head = head < V ? head : V;
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;

    float mx = -INFINITY;
    if (tid < head) mx = row[tid];
    for (int f = tid; f < n4; f += 256) {
        const float4 v = ld4(row + head + 4 * f);
        mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    if (tail0 + tid < V) mx = fmaxf(mx, row[tail0 + tid]);
    mx = wave_max(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();   // s_red is reused below

    float sum = 0.f;
    if (tid < head) sum = expf(row[tid] - mx);
    for (int f = tid; f < n4; f += 256) {
        const float4 v = ld4(row + head + 4 * f);
        sum += (expf(v.x - mx) + expf(v.y - mx)) + (expf(v.z - mx) + expf(v.w - mx));
    }
    if (tail0 + tid < V) sum += expf(row[tail0 + tid] - mx);
    sum = wave_sum(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (tid == 0) out[m] = (row[tgt] - mx) - logf(((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]);
}

int launch_logprob_gather(const float* logits, int64_t ld, const int32_t* targets, float* out, int M, int V, hipStream_t st) {
    MGEA_REQUIRE(logits && targets && out && M > 0 && V > 0 && ld >= V, MGEA_EINVAL, "logprob_gather: bad argument (M=%d V=%d ld=%lld)", M, V,
                 (long long)ld);
    hipLaunchKernelGGL(logprob_gather_kernel, dim3(M), dim3(256), 0, st, logits, ld, targets, out, V);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
