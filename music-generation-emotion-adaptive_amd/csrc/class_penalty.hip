// Windowed penalties over token classes (include/mgea.h, mgea_row_class_penalty): the launch behind the guidance and blend mixes and in
// front of the sampler of a class-penalised decode step.  class_of [V] maps every id to a class in [-1, n_class) (-1 = in no class);
// row b counts the classes of the ids its last `window` steps took, n_c, and every id i of a counted class gets
//   m = frequency * (float)n_c,  d = m + presence,  x[i] = x[i] - d      (three separately rounded fp32 operations)
// Everything else -- finished rows, rows whose record is off, t == 0, ids of class -1, ids of classes with n_c == 0 -- is not written.
#include "common.h"

namespace mgea {

constexpr int CPEN_NT = 256;   // threads per row: the sampler's geometry

// The rule's three operations, each rounded to nearest on its own.  HIP's __fmul_rn / __fadd_rn / __fsub_rn are a plain *, + and - whose
// instructions carry the default -ffp-contract=fast of the header they are defined in, so the compiler fuses the first two into one
// v_fma_f32 (ONE rounding; seen in the assembly and as wrong last bits against the host rule).  Under this pragma the operations
// carry no licence to contract, and the kernel below has a v_mul_f32, a v_add_f32 and a v_sub_f32.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

// One CPEN_NT-thread workgroup per batch row; the grid is B whatever the records say, so the captured step graph does not depend on
// them.  The exit test reads the row's own done word, record and step: block-uniform, in front of every barrier.
// The counters are n_class 32-bit words of dynamic LDS (at most MGEA_SAMPLER_MAX_VOCAB = 14336 words, 56 KB).  Threads stride over the
// window [lo, t) of the row's id history: an entry outside [0, V) is skipped, never used as an index, and so is a class outside
// [0, n_class); the count is an integer LDS atomic add, so the result does not depend on the order the waves arrive in.  The history
// is read at j < t <= stride only.  Then threads stride over the ids with coalesced reads of the map (shared by all rows: L2-resident)
// and read-modify-write x[i] only where the id's class was counted.  No float atomics, nothing between workgroups: row b's workgroup
// is the only one that touches row b.
__global__ __launch_bounds__(CPEN_NT) void class_penalty_kernel(float* __restrict__ logits, int V, const int32_t* __restrict__ class_of,
                                                                int n_class, const int32_t* __restrict__ hist, int stride,
                                                                const int32_t* __restrict__ row_step, const int32_t* __restrict__ done,
                                                                const mgea_row_class_penalty* __restrict__ recs) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cpen_count[];   // [n_class]
    const int b = blockIdx.x, tid = threadIdx.x;
    if (done[b] != 0) return;
    const mgea_row_class_penalty rec = recs[b];
    if (!(rec.frequency != 0.f || rec.presence != 0.f)) return;
    int t = row_step[b];
    t = t < stride ? t : stride;
    if (t <= 0) return;
    const int lo = rec.window > 0 && t > rec.window ? t - rec.window : 0;
    for (int c = tid; c < n_class; c += CPEN_NT) cpen_count[c] = 0u;
    __syncthreads();
    const int32_t* h = hist + (int64_t)b * stride;
    for (int j = lo + tid; j < t; j += CPEN_NT) {
        const int32_t id = h[j];
        if ((uint32_t)id >= (uint32_t)V) continue;
        const int32_t c = class_of[id];
        if ((uint32_t)c < (uint32_t)n_class) atomicAdd(&cpen_count[c], 1u);
    }
    __syncthreads();
    float* x = logits + (int64_t)b * V;
    for (int i = tid; i < V; i += CPEN_NT) {
        const int32_t c = class_of[i];
        if ((uint32_t)c >= (uint32_t)n_class) continue;
        const uint32_t n = cpen_count[c];
        if (n == 0u) continue;
        const float m = mul_rn(rec.frequency, (float)n);
        const float d = add_rn(m, rec.presence);
        x[i] = sub_rn(x[i], d);
    }
}

int launch_class_penalty(float* logits, int B, int V, const int32_t* class_of, int n_class, const int32_t* hist, int stride,
                         const int32_t* row_step, const int32_t* done, const mgea_row_class_penalty* recs, hipStream_t st) {
    MGEA_REQUIRE(logits && class_of && hist && row_step && done && recs && B > 0, MGEA_EINVAL, "class penalty: NULL argument or empty batch");
    MGEA_REQUIRE(V > 0 && V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "class penalty: vocab %d exceeds the sampler's row (%d)", V,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(n_class >= 1 && n_class <= V, MGEA_EINVAL, "class penalty: n_class %d outside [1, %d]", n_class, V);
    MGEA_REQUIRE(stride > 0, MGEA_EINVAL, "class penalty: history stride %d must be > 0", stride);
    static_assert(MGEA_SAMPLER_MAX_VOCAB * sizeof(uint32_t) <= 64 * 1024, "the counters of the identity map must fit one workgroup's LDS");
    const int shmem = n_class * (int)sizeof(uint32_t);
    if (shmem > 32 * 1024) {   // above the default limit of a launch: raised once per device
        DeviceInfo di;
        MGEA_TRY(device_info(&di));
        static uint64_t attr_done = 0;
        MGEA_TRY(set_max_dynamic_lds((const void*)class_penalty_kernel, MGEA_SAMPLER_MAX_VOCAB * (int)sizeof(uint32_t), di.dev, &attr_done));
    }
    hipLaunchKernelGGL(class_penalty_kernel, dim3(B), dim3(CPEN_NT), shmem, st, logits, V, class_of, n_class, hist, stride, row_step, done, recs);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
