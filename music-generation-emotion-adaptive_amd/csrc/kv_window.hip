// The sliding KV window of a generation that outruns its reservation (include/mgea.h, mgea_decoder_set_window): the kernel that
// opens a windowed decode step.  Every row keeps P = S + R logical pages: 0 .. S-1 are the sink (the prompt: never evicted), S .. P-1
// a ring.  A row that is not finished and whose ctx_len == 64 P - 1 at the start of a step gives up its oldest ring page whole.
#include "common.h"

namespace mgea {

// One wave per row.  On the trigger the row's entries [S, P) rotate left by one -- the freed physical page becomes logical page
// P-1 --, ctx_len drops by a page and the row's eviction counter goes up by one (a plain word: this wave is its only writer).  A row
// off the trigger stores nothing.  Every load of the row's entries is issued before the first store: the ring (<= WINDOW_MAX_RING
// entries, checked by the launcher) sits in WINDOW_CHUNKS registers per lane.  No other wave touches the row, so nothing is ordered
// across waves; the kernels of the step behind this one read the table in stream order.
// Why 64 P - 1 and not 64 P: with the qkv0 table the PREVIOUS step's tail has already stored layer 0's K | V of the token this step
// feeds at logical position ctx_len = 64 P - 1, the last slot of logical page P-1.  The rotation moves that page to P-2 and ctx_len
// to 64 P - 65, its last slot: the write stays in bounds and stays where this step's attention reads it.
constexpr int WINDOW_CHUNKS = WINDOW_MAX_RING / 64;
__global__ __launch_bounds__(64) void window_evict_kernel(int32_t* __restrict__ page_table, int max_pages, int S, int P,
                                                          int32_t* __restrict__ ctx_len, const int32_t* __restrict__ done,
                                                          int32_t* __restrict__ evictions) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int len = ctx_len[b];
    if (done[b] || len != P * MGEA_KV_PAGE_TOKENS - 1) return;   // (a whole-wave decision: both are the row's values)
    int32_t* row = page_table + (int64_t)b * max_pages;
    const int n_ev = evictions[b];
    int32_t v[WINDOW_CHUNKS];
#pragma unroll
    for (int c = 0; c < WINDOW_CHUNKS; ++c) {
        const int j = S + c * 64 + lane;             // the logical page this lane rewrites
        const int src = j + 1 < P ? j + 1 : S;       // its left-rotated source: the next one, the oldest for the last
        v[c] = j < P ? row[src] : 0;
    }
#pragma unroll
    for (int c = 0; c < WINDOW_CHUNKS; ++c) {
        const int j = S + c * 64 + lane;
        if (j < P) row[j] = v[c];
    }
    if (lane == 0) {
        ctx_len[b] = len - MGEA_KV_PAGE_TOKENS;
        evictions[b] = n_ev + 1;
    }
}

int launch_window_evict(int32_t* page_table, int max_pages, int S, int R, int32_t* ctx_len, const int32_t* done, int32_t* evictions,
                        int B, hipStream_t st) {
    MGEA_REQUIRE(page_table && ctx_len && done && evictions && B > 0, MGEA_EINVAL, "window evict: NULL argument or empty batch");
    MGEA_REQUIRE(S >= 1, MGEA_EINVAL, "window evict: sink_pages %d must be >= 1", S);
    MGEA_REQUIRE(R >= 2 && R <= WINDOW_MAX_RING, MGEA_EINVAL, "window evict: ring_pages %d outside [2, %d]", R, WINDOW_MAX_RING);
    MGEA_REQUIRE((int64_t)S + R <= max_pages, MGEA_EINVAL, "window evict: sink_pages %d + ring_pages %d exceed the %d pages of a row", S, R,
                 max_pages);
    hipLaunchKernelGGL(window_evict_kernel, dim3(B), dim3(64), 0, st, page_table, max_pages, S, S + R, ctx_len, done, evictions);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
