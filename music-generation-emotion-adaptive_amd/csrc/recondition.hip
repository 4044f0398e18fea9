// Emotion transitions (include/mgea.h, mgea_row_schedule): a row's prompt K | V swapped in the middle of a generation.  Decode steps
// use position row 0 and the attention is mask-free over the cache, so "the model now sees prompt variant s" IS "the K | V of cache
// positions [0, len_b) of every layer are those a prefill of variant s caches".  Two kernels: cond_gather_kernel copies those positions
// out of the pages of a prefill that has just finished into the CONDITIONING STORE, cond_apply_kernel opens every scheduled decode
// step and, for the rows whose segment has changed, copies the new variant's positions back over the row's pages.  Both move 16-byte
// groups in the page's element type (4 floats / 8 halves: the K page's group G) and never look inside one, so one kernel serves the
// fp32 and the fp16 pool; nothing is rounded, the pages end up bit for bit as the variant's own prefill left them.
//
// The store: [n_seg_max][n_layer][B][slot], slot = 2 * H * (dh / G) * slot_tokens groups.  A row of length len fills the first
// n = 2 * H * D * len groups of its slot (D = dh / G), packed in the order the apply kernel's threads walk them, so that thread i of
// a round loads group i: consecutive bytes.
//   i <  n / 2  (K):  i = (h * D + dg) * len + t   <->  group dg * 64 + t of head h's K page   ([dh / G][64][G])
//   i >= n / 2  (V):  j = i - n / 2 = h * len * D + r, r = t * D + dg   <->  group r of head h's V page   ([64][dh])
// The layout's three numbers (slot_tokens, B, n_seg_max) live in device memory next to the store (meta, written by the gather), so a
// captured step does not depend on the call's prompt width or segment count.
#include "common.h"

namespace mgea {

constexpr int COND_NT = 256;      // threads per row
constexpr int COND_ROUND = 16;    // groups per thread whose loads are all in flight before the round's first store (64 VGPRs)

// one 16-byte group, moved whole (a native vector: a round of HIP's uint4 structs is not kept in registers, 272 bytes of scratch a lane)
typedef unsigned int g16 __attribute__((ext_vector_type(4)));

namespace {
struct CondGeom {
    int H, D, len, half;          // heads, 16-byte groups per token and head, the row's prompt length, n / 2
    int64_t page_groups;          // groups of one head's K (or V) page: 64 * D
};
// group i of a row's slot -> its group offset from the start of the row's physical page (K of head 0) in one layer
__device__ __forceinline__ int64_t cond_page_off(const CondGeom& g, int i) {
    const int isv = i >= g.half;
    const int j = isv ? i - g.half : i;
    const int per_head = g.D * g.len;
    const int h = j / per_head, r = j - h * per_head;
    int in_page = r;                                   // V: [64 tokens][D]
    if (!isv) {
        const int dg = r / g.len, t = r - dg * g.len;  // K: [D][64 tokens]
        in_page = dg * MGEA_KV_PAGE_TOKENS + t;
    }
    return ((int64_t)isv * g.H + h) * g.page_groups + in_page;
}
// the physical page of row b's logical page 0: the decoder's allocation rule where the pool carries it, the table otherwise
__device__ __forceinline__ int cond_phys(const KvPool& pool, const int32_t* page_table, int max_pages, int b) {
    return pool.arith_batch > 0 ? b : page_table[(int64_t)b * max_pages];
}
}  // namespace

// grid (B, n_layer): the pages of row b, layer l -> slot (seg, l, b).  Block (0, 0) also files the layout and every layer-0 block its
// row's length: the apply kernel reads both from device memory.
__global__ __launch_bounds__(COND_NT) void cond_gather_kernel(KvPool pool, const int32_t* __restrict__ page_table, int max_pages,
                                                              const int32_t* __restrict__ lens, int Tp, g16* __restrict__ store,
                                                              int seg, int n_seg_max, int slot_tokens, int32_t* __restrict__ meta,
                                                              int32_t* __restrict__ cond_len) {
    const int b = blockIdx.x, l = blockIdx.y, B = gridDim.x, L = gridDim.y, tid = threadIdx.x;
    int len = lens ? lens[b] : Tp;
    len = len < 0 ? 0 : len > slot_tokens ? slot_tokens : len;   // (the hosts check lens; a stray word must not leave the slot)
    const int phys = cond_phys(pool, page_table, max_pages, b);
    if (tid == 0) {
        if (l == 0) cond_len[b] = len;
        if (l == 0 && b == 0) {
            meta[0] = slot_tokens; meta[1] = B; meta[2] = n_seg_max; meta[3] = 0;
        }
    }
    if (phys < 0 || phys >= pool.n_pages) return;
    const int G = pool.f16 ? 8 : 4;
    CondGeom g;
    g.H = pool.H; g.D = pool.dh / G; g.len = len; g.half = g.H * g.D * len;
    g.page_groups = (int64_t)MGEA_KV_PAGE_TOKENS * g.D;
    const int n = 2 * g.half;
    const g16* page = static_cast<const g16*>(pool.base) + (l * pool.layer_stride) / G + (int64_t)phys * 2 * g.H * g.page_groups;
    g16* slot = store + (((int64_t)seg * L + l) * B + b) * ((int64_t)2 * g.H * g.D * slot_tokens);
    for (int i0 = 0; i0 < n; i0 += COND_NT * COND_ROUND) {
        g16 v[COND_ROUND];
#pragma unroll
        for (int r = 0; r < COND_ROUND; ++r) {
            const int i = i0 + r * COND_NT + tid;
            if (i < n) v[r] = page[cond_page_off(g, i)];
        }
#pragma unroll
        for (int r = 0; r < COND_ROUND; ++r) {
            const int i = i0 + r * COND_NT + tid;
            if (i < n) slot[i] = v[r];
        }
    }
}

// One COND_NT-thread workgroup per batch row (grid = B): the row's cur_seg word has one reader-writer, nothing is exchanged between
// workgroups.  The row's finished flag, both keys, the record, cur_seg and the layout are requested in ONE batch of loads -- all the
// row's own words, so the compiler makes them scalar loads and the decision is block-uniform -- and a row whose segment stands
// returns: the common case is those loads and a branch (the length and, on the table path, the page id are only needed behind it and
// are requested there).  Otherwise, layer by layer, slot (seg, l, b) goes back over the row's page in rounds of COND_ROUND
// groups per thread, every load of a round issued before its first store (a whole layer for prompts of up to 16 tokens at
// d_model 512 in fp32).  Thread 0 then stores cur_seg behind a barrier -- after every thread's stores are issued -- and counts the
// switch.  Positions >= len_b, ctx_len, cur_ids, the histories and every sampler input are never touched.
__global__ __launch_bounds__(COND_NT) void cond_apply_kernel(KvPool pool, int n_layer, const int32_t* __restrict__ page_table,
                                                             int max_pages, const g16* __restrict__ store,
                                                             const int32_t* __restrict__ meta, const int32_t* __restrict__ cond_len,
                                                             const mgea_row_schedule* __restrict__ sched,
                                                             const int32_t* __restrict__ done, const int32_t* __restrict__ row_step,
                                                             const int32_t* __restrict__ gram_state, int32_t* __restrict__ cur_seg,
                                                             int32_t* __restrict__ switches) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int fin = done[b], k_step = row_step[b], k_state = gram_state[b], cur = cur_seg[b];
    const mgea_row_schedule rec = sched[b];
    const int4 lay = *reinterpret_cast<const int4*>(meta);   // slot_tokens, B, n_seg_max
    const int k = rec.key ? k_state : k_step;
    int seg = 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) seg += (int)(s < rec.n_segments - 1) & (int)(rec.threshold[s] <= k);
    // one decision over everything loaded above (no branch between the loads: they stay one batch); a finished or parked row never switches
    if ((int)(fin != 0) | (int)(seg == cur)) return;
    int len = cond_len[b];
    const int phys = cond_phys(pool, page_table, max_pages, b);
    // (the hosts check all of these; a stray word must not reach memory)
    if (seg >= lay.z || b >= lay.y || phys < 0 || phys >= pool.n_pages || len < 1) return;
    len = len > lay.x ? lay.x : len;
    const int G = pool.f16 ? 8 : 4;
    CondGeom g;
    g.H = pool.H; g.D = pool.dh / G; g.len = len; g.half = g.H * g.D * len;
    g.page_groups = (int64_t)MGEA_KV_PAGE_TOKENS * g.D;
    const int n = 2 * g.half;
    const int64_t slot_groups = (int64_t)2 * g.H * g.D * lay.x;
    for (int l = 0; l < n_layer; ++l) {
        g16* page = static_cast<g16*>(pool.base) + (l * pool.layer_stride) / G + (int64_t)phys * 2 * g.H * g.page_groups;
        const g16* slot = store + (((int64_t)seg * n_layer + l) * lay.y + b) * slot_groups;
        for (int i0 = 0; i0 < n; i0 += COND_NT * COND_ROUND) {
            g16 v[COND_ROUND];
#pragma unroll
            for (int r = 0; r < COND_ROUND; ++r) {
                const int i = i0 + r * COND_NT + tid;
                if (i < n) v[r] = slot[i];
            }
#pragma unroll
            for (int r = 0; r < COND_ROUND; ++r) {
                const int i = i0 + r * COND_NT + tid;
                if (i < n) page[cond_page_off(g, i)] = v[r];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        cur_seg[b] = seg;
        atomicAdd(switches, 1);
    }
}

namespace {
int check_cond_pool(const KvPool& pool, int n_layer, const int32_t* page_table, int max_pages, const char* who) {
    MGEA_REQUIRE(pool.base && n_layer > 0 && pool.n_pages > 0 && pool.H > 0, MGEA_EINVAL, "%s: NULL pool or empty geometry", who);
    MGEA_REQUIRE(pool.dh == 32 || pool.dh == 64 || pool.dh == 96, MGEA_EINVAL, "%s: head_dim %d not supported (32, 64 or 96)", who, pool.dh);
    MGEA_REQUIRE(pool.f16 == 0 || pool.f16 == 1, MGEA_EINVAL, "%s: bad element type", who);
    MGEA_REQUIRE(pool.layer_stride == (int64_t)pool.n_pages * 2 * pool.H * pool.page_elems(), MGEA_EINVAL, "%s: layer stride %lld is not that of %d pages",
                 who, (long long)pool.layer_stride, pool.n_pages);
    MGEA_REQUIRE(pool.arith_batch >= 0 && pool.arith_batch <= pool.n_pages, MGEA_EINVAL, "%s: arith_batch %d outside [0, %d]", who, pool.arith_batch,
                 pool.n_pages);
    MGEA_REQUIRE(pool.arith_batch > 0 || (page_table && max_pages >= 1), MGEA_EINVAL, "%s: neither the allocation rule nor a page table", who);
    return MGEA_OK;
}
}  // namespace

int64_t cond_store_bytes(const KvPool& pool, int n_layer, int n_seg_max, int B, int slot_tokens) {
    return (int64_t)n_seg_max * n_layer * B * 2 * pool.H * pool.dh * slot_tokens * pool.elt_bytes();
}

int launch_cond_gather(const KvPool& pool, int n_layer, const int32_t* page_table, int max_pages, const int32_t* lens, int Tp, void* store,
                       int seg, int n_seg_max, int slot_tokens, int32_t* meta, int32_t* cond_len, int B, hipStream_t st) {
    MGEA_TRY(check_cond_pool(pool, n_layer, page_table, max_pages, "cond gather"));
    MGEA_REQUIRE(store && meta && cond_len && B > 0, MGEA_EINVAL, "cond gather: NULL argument or empty batch");
    MGEA_REQUIRE(pool.arith_batch == 0 || B <= pool.arith_batch, MGEA_EINVAL, "cond gather: %d rows beyond the allocation rule's %d", B, pool.arith_batch);
    MGEA_REQUIRE(n_seg_max >= 1 && n_seg_max <= MGEA_SCHEDULE_MAX_SEGMENTS && seg >= 0 && seg < n_seg_max, MGEA_EINVAL,
                 "cond gather: segment %d of %d (at most %d)", seg, n_seg_max, MGEA_SCHEDULE_MAX_SEGMENTS);
    MGEA_REQUIRE(slot_tokens >= 1 && slot_tokens <= MGEA_KV_PAGE_TOKENS && Tp >= 1 && Tp <= slot_tokens, MGEA_EINVAL,
                 "cond gather: prompt width %d / slot of %d tokens (at most one page of %d)", Tp, slot_tokens, MGEA_KV_PAGE_TOKENS);
    hipLaunchKernelGGL(cond_gather_kernel, dim3(B, n_layer), dim3(COND_NT), 0, st, pool, page_table, max_pages, lens, Tp,
                       static_cast<g16*>(store), seg, n_seg_max, slot_tokens, meta, cond_len);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

int launch_cond_apply(const KvPool& pool, int n_layer, const int32_t* page_table, int max_pages, const void* store, const int32_t* meta,
                      const int32_t* cond_len, const mgea_row_schedule* sched, const int32_t* done, const int32_t* row_step,
                      const int32_t* gram_state, int32_t* cur_seg, int32_t* switches, int B, hipStream_t st) {
    MGEA_TRY(check_cond_pool(pool, n_layer, page_table, max_pages, "cond apply"));
    MGEA_REQUIRE(store && meta && cond_len && sched && done && row_step && gram_state && cur_seg && switches && B > 0, MGEA_EINVAL,
                 "cond apply: NULL argument or empty batch");
    MGEA_REQUIRE(pool.arith_batch == 0 || B <= pool.arith_batch, MGEA_EINVAL, "cond apply: %d rows beyond the allocation rule's %d", B, pool.arith_batch);
    hipLaunchKernelGGL(cond_apply_kernel, dim3(B), dim3(COND_NT), 0, st, pool, n_layer, page_table, max_pages, static_cast<const g16*>(store),
                       meta, cond_len, sched, done, row_step, gram_state, cur_seg, switches);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

}  // namespace mgea
