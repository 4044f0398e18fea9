// The 16-bit flash attention of the perf modes (bf16: DistilBERT; fp16: the decoder's big-batch prefill, which also writes the K | V
// pages from here), head_dim 64.
// * attn_bf16_kernel: persistent, LDS-DMA double-buffered flash attention over a packed 16-bit qkv buffer with an optional key
//   mask; S^T = K Q^T keeps the query on lane&15, so the softmax is in-lane + two permlane swaps and the fp32 accumulators,
//   converted to 16 bits, ARE the B operand of O^T = V^T P^T (k-permutation shared by V^T, which is read with ds_read_b64_tr_b16).
// * launch_attn16 / launch_attn_bf16: <4 waves, 128 keys> or <8 waves, 256 keys> per stage, rolled or software-pipelined.
#include "x16.h"

namespace mgea {

// In-kernel time stamps of the attention's units (cdna_hip_programming.md section 7), compiled ONLY into the tools build
// (tools/build_stamps.sh: -DMGEA_PH_STAMPS, a separate .so that tools/attn_stamps.py loads); the product library has none of it.
#ifdef MGEA_PH_STAMPS
__device__ unsigned long long* g_attn_stamps = nullptr;    // [workgroup][64] 100 MHz ticks, written by thread 0
#define PH_STAMP(i) do { if (g_attn_stamps && tid == 0 && (i) < 64) g_attn_stamps[(size_t)blockIdx.x * 64 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int mgea_dbg_set_attn_stamps(unsigned long long* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_stamps), &p, sizeof(p)); }
#else
#define PH_STAMP(i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------
// Reductions over the four lanes c, c + 16, c + 32, c + 48 (the lanes that share a query in the K Q^T accumulator) with gfx950's
// v_permlane32_swap / v_permlane16_swap: VALU instructions, no trip through the LDS pipeline like ds_bpermute (__shfl_xor), which
// matters at 2 waves per SIMD where nothing hides that latency.  swap(x, x) leaves [lo, lo] / [hi, hi] (32) or [r0 r0 r2 r2] / [r1 r1
// r3 r3] (16) in the two results, so one max of the pair is the xor-32 / xor-16 butterfly step.
// max(a, b) as the median of (a, b, +inf): ONE v_med3_f32.  fmaxf() on values that come out of an MFMA or a lane swap costs two extra
// instructions each -- hipcc canonicalises both inputs first (v_max_f32 x, x, x: IEEE maxNum semantics for signalling NaNs), 16 + 8 of them
// per 64-key tile of the flash attention.  No score is a NaN here; -inf (masked keys) orders as usual.
__device__ __forceinline__ float max_nc(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, INFINITY); }
__device__ __forceinline__ float quad_max(float x) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float m = max_nc(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return max_nc(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// ------------------------------------------------------------------------------------------
// Flash attention, bf16 in/out, head_dim 64.  PERSISTENT and software-pipelined: 2 workgroups per CU walk the work items
// (b, h, block of 128 queries); 4 waves x 32 queries (two 16-query MFMA column blocks per wave, every V fragment read from LDS feeds
// two MFMAs).  Keys are staged 128 at a time -- for the DistilBERT shape (T = 128) K and V of a (b, h) leave HBM exactly once --
// by LDS-DMA into one of two 32 KB stages: the DMA of unit u + 1 is issued right after the barrier that opens unit u and flies under
// u's MFMAs, softmax and output stores.  (Without it every workgroup of a round loads, computes and stores in step with all the
// others: 54 us = 27 load + 16 + 11, the phases add up.)  The DMA is issued from inline asm (glds16_hidden) so that hipcc does not
// drain vmcnt in front of every LDS read; the only wait for it is the explicit vmcnt(0) at the top of a unit, where nothing younger
// is in flight.
//   K image [key][8 x 16 B], chunk ^= key & 7            : row reads (ds_read_b128) for the A operand of K Q^T, conflict-free
//   V image [key][8 x 16 B], chunk ^= ((key >> 1) & 3) * 2: read with ds_read_b64_tr_b16, the hardware transpose (guide T10): lanes
//      16g..16g+15 fetch a block of 4 keys x 16 d and lane c gets column d = 16 dt + c of the 4 keys -- the V^T A-operand of the
//      P V product without a transposing write pass.  The 8 rows a 32-lane half touches land on 8 different 8-bank groups.
//   Both swizzles are applied on the GLOBAL side of the DMA (a lane picks which 16 bytes of its key's row it fetches); the LDS side
//   of a DMA is lane-linear.  EXEC is all ones at every transposed read (uniform control flow only).
// S^T = K Q^T keeps a query's scores lane-local (lane = query, registers = keys 16 kt + 4 g + r); the k index of the P V product is
// permuted to match (k = 8 g + j  <->  key 32 p + 16 (j >> 2) + 4 g + (j & 3)), so P goes from accumulator to operand in registers.
// The output tile goes through the (then free) K image so that every store instruction writes complete 128-byte rows.
// NW waves x 32 queries per workgroup, keys staged KB = 32 NW at a time: <4, 128> (two workgroups per CU) for short sequences -- DistilBERT: K and V
// of a (batch, head) leave HBM exactly once --, <8, 256> (one workgroup per CU, 2 x 64 KB stages) for long ones, where the per-unit costs (the
// wait for the DMA, the barrier, 8 LDS-DMA pieces per wave: 1.7 of 4.3 us per unit by in-kernel stamps at 1024 keys) are spread over four
// 64-key tiles instead of two.
template <typename E, int NW, int PIPE>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2)))
void attn_bf16_kernel(const E* __restrict__ qkv, const int32_t* __restrict__ mask, E* __restrict__ out, int T, int H,
                      int n_items, int nqb, float scale, KvPages pg, const int32_t* __restrict__ cu) {
    typedef typename X16<E>::v8 bf16x8;   // (the names below were written for bf16; E may be _Float16)
    typedef typename X16<E>::v4 bf16x4;
    typedef E bf16_t;
    constexpr int DH = 64, KB = 32 * NW, QPB = 32 * NW;           // keys per stage, queries per workgroup
    constexpr int STAGE = KB * 16;                                // 16-byte chunks: K image [KB][8], then V image [KB][8]
    constexpr int VW = KB / 64;                                   // 64-bit validity words per stage
    extern __shared__ __attribute__((aligned(16))) float4 lds[];  // [2][STAGE], then [2][VW] 64-bit validity words
    unsigned long long* sValid = reinterpret_cast<unsigned long long*>(lds + 2 * STAGE);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float4*)lds;

    const int C = H * DH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int nkb = (T + KB - 1) / KB;
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

    // DMA of one unit (item, key block) into a stage: wave w moves keys 32 w .. 32 w + 31 of K and of V (8 instructions of 1 KB)
    const int d_key = lane >> 3, d_ch = lane & 7;                 // this lane's slot inside an 8-key piece
    const unsigned dk_off = 2u * C + 16u * (d_ch ^ d_key);                              // K: chunk ^ (key & 7), key & 7 == d_key
    const unsigned dv_off = 4u * C + 16u * (d_ch ^ (((d_key >> 1) & 3) << 1));          // V: chunk ^ 2 ((key >> 1) & 3)
    // PACKED ("varlen") INPUT, cu != NULL (round 4, DistilBERT on unpadded batches): the rows of sequence b are cu[b] .. cu[b + 1] - 1 of one
    // [sum of lengths, 3 C] buffer, no padding rows and no key mask; every sequence fits one query block and one key stage (host check:
    // max length <= KB, so nqb == nkb == 1 and an item is a (sequence, head)).  T then only sizes the grid; a sequence's own length
    // bounds its key tiles, so a 20-token prompt computes one 64-key tile where the padded form computes the batch's maximum.
    auto seq_rows = [&](int bb, int& row0, int& Tb) {            // wave-uniform (scalar loads)
        if (cu) { row0 = cu[bb]; Tb = cu[bb + 1] - row0; } else { row0 = bb * T; Tb = T; }
    };
    struct ItemBase { const bf16_t* p; int Tb; };
    auto item_base = [&](int it) {                                // first qkv row of the item's (batch, head): wave-uniform, stays in SGPRs
        const int bh = it / nqb, bb = bh / H, hh = bh - bb * H;
        int row0, Tb;
        seq_rows(bb, row0, Tb);
        return ItemBase{qkv + (int64_t)row0 * 3 * C + hh * DH, Tb};
    };
    auto issue_part = [&](const ItemBase& ib, int kbi, int st, int i0, int i1) {   // pieces i0 .. i1 - 1 of this wave's four (K and V of 8 keys each)
        const bf16_t* base = ib.p;
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            const int piece = wave * 4 + i, key = piece * 8 + d_key;
            int kr = kbi * KB + key; kr = kr < ib.Tb ? kr : ib.Tb - 1;
            const unsigned row = (unsigned)kr * (unsigned)(6 * C);    // bytes; a sequence's rows span < 4 GB (checked on the host)
            const unsigned dst = lds_base + (unsigned)(st * STAGE + piece * 64) * 16u;
            glds16_hidden_s(base, row + dk_off, dst);
            glds16_hidden_s(base, row + dv_off, dst + (unsigned)(KB * 8) * 16u);
        }
    };
    auto issue = [&](int it, int kbi, int st) { issue_part(item_base(it), kbi, st, 0, 4); };
    auto mask_of = [&](int it, int kbi) -> int {                  // validity of key kbi * KB + tid (the first KB / 64 waves)
        const int bh = it / nqb, bb = bh / H;
        const int kidx = kbi * KB + tid;
        int row0, Tb;
        seq_rows(bb, row0, Tb);
        int ok = (tid < KB && kidx < Tb) ? 1 : 0;
        if (ok && mask) ok = mask[(int64_t)bb * T + kidx];        // (packed input has no mask: host check)
        return ok;
    };
    bf16x8 qn[2][2];                                              // next item's raw Q fragments
    auto load_q = [&](int it) {
        const int bh = it / nqb, qb = it - bh * nqb, bb = bh / H, hh = bh - bb * H;
        int row0, Tb;
        seq_rows(bb, row0, Tb);
#pragma unroll
        for (int mq = 0; mq < 2; ++mq) {
            int qr = qb * QPB + wave * 32 + mq * 16 + c; qr = qr < Tb ? qr : Tb - 1;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                qn[mq][ks] = *reinterpret_cast<const bf16x8*>(qkv + ((int64_t)row0 + qr) * 3 * C + hh * DH + ks * 32 + 8 * g);
        }
    };
    // transposed-read offsets (bf16 elements) of this lane inside a 16-key group of the V image, one per 16-d block:
    // row 4 g + (c >> 2) of the group, 16-byte chunk (2 dt + ((c & 3) >> 1)) ^ swizzle(row), half (c & 1)
    int v_off[4];
    {
        const int vrow = 4 * g + (c >> 2), sw = ((vrow >> 1) & 3) << 1;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) v_off[dt] = vrow * 64 + (((2 * dt + ((c & 3) >> 1)) ^ sw) * 8) + 4 * (c & 1);
    }

    // The output rows of an item are held in registers and stored one unit later, behind the next DMA issue: a store issued at the
    // end of a unit would be waited for (vmcnt(0), loads and stores share the counter) at the top of the next one with nothing to hide
    // its latency behind -- 2-3 us per item.
    float4 ov0, ov1, ov2, ov3;                                    // (scalars, not an array: an array captured by a lambda went to scratch)
    bf16_t* optr = nullptr;                                       // row of ov0; ov<i> is 8 i rows further; nullptr: nothing held
    int orow = 0, oT = 0;                                         // query index of ov0 within the sequence, and that sequence's length
#define MGEA_FLUSH_OUT()                                                                               \
    if (optr) {                                                                                        \
        if (orow < oT)      *reinterpret_cast<float4*>(optr) = ov0;                                    \
        if (orow + 8 < oT)  *reinterpret_cast<float4*>(optr + (int64_t)8 * C) = ov1;                   \
        if (orow + 16 < oT) *reinterpret_cast<float4*>(optr + (int64_t)16 * C) = ov2;                  \
        if (orow + 24 < oT) *reinterpret_cast<float4*>(optr + (int64_t)24 * C) = ov3;                  \
    }
    int item = blockIdx.x, kb = 0, stage = 0, mk = 0;
    if (item < n_items) { issue(item, 0, 0); mk = mask_of(item, 0); load_q(item); }
    bf16x8 qf[2][2];
    f32x4 oacc[2][4], lacc[2];                                    // lacc: row sums of P, from an all-ones A operand (every row equal)
    float mx[2];                                                  // running maximum of the RAW scores q . k
    const float kexp = scale * 1.4426950408889634f;               // exp(scale * (s - m)) = 2^((s - m) * kexp)
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (bf16_t)1.0f;
    [[maybe_unused]] int un = 0;                                   // (tools-only stamps: unit counter)
    while (item < n_items) {
        PH_STAMP(un * 8 + 0);
        // unit (item, kb) has landed: nothing younger than its DMA, its mask word and (kb == 0) its Q rows is in flight here
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PH_STAMP(un * 8 + 1);
        // Tell hipcc that the prefetched registers are complete on every path.  It does not read the wait above, and a load it still
        // believes pending makes it wait (by ITS count, which does not include the hidden DMAs: in effect vmcnt(0)) before those
        // registers are written again -- right after the next unit's DMA was issued, which would serialise the pipeline.
        asm volatile("" : "+v"(qn[0][0]), "+v"(qn[0][1]), "+v"(qn[1][0]), "+v"(qn[1][1]), "+v"(mk));
        int row0cur, Tcur;                                        // the current item's sequence: first row, length
        seq_rows((item / nqb) / H, row0cur, Tcur);
        if (tid < KB) {
            const unsigned long long bal = __ballot(mk != 0);
            if (lane == 0) sValid[stage * VW + wave] = bal;
        }
        __syncthreads();
        PH_STAMP(un * 8 + 2);
        if (kb == 0) {
#pragma unroll
            for (int mq = 0; mq < 2; ++mq) {
                mx[mq] = -INFINITY;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) oacc[mq][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                lacc[mq] = (f32x4){0.f, 0.f, 0.f, 0.f};
                qf[mq][0] = qn[mq][0];                               // unscaled: 1/sqrt(dh) is folded into the exponent's constant
                qf[mq][1] = qn[mq][1];
            }
        }
        // K | V OF THE REAL TOKENS -> fp16 KV PAGES (decoder prefill, round 4; replaces kv_scatter_f16_kernel, which re-read the K | V columns
        // of the qkv buffer from HBM -- 134 MB in, 134 MB out per layer at [64, 1024]).  The stage that has just landed holds exactly
        // those rows: ONE of the (batch, head)'s items writes them out (below), each wave the 32 keys it moved in -- K as
        // [d-group][token][8 halves] (lane = token: 512 contiguous bytes per d-group and instruction), V as whole 128-byte rows.
        // Only keys with their validity bit set (t < lens[b], t < T) are cached, at position t (the cache is empty: run_prefill16).
        if constexpr (sizeof(E) == 2 && !X16<E>::is_bf16) {
            if (pg.pool.base) {
                const int bh_u = item / nqb, qb_u = item - bh_u * nqb;
                if (qb_u == kb) {     // (nqb == nkb: queries per item = keys per stage.  The item of query block kb writes key block kb -- every
                                      //  workgroup a quarter of the stages; with query block 0 writing all of them a quarter of the workgroups
                                      //  did all the writing and the launch waited for them: 4.64 ms per cache fill against 4.37 with the scatter kernel)
                    const int bb = bh_u / H, hh = bh_u - bb * H;
                    const int tok0 = kb * KB + wave * 32;                                   // 32-aligned: one page
                    const unsigned long long vw = sValid[stage * VW + (wave >> 1)];
                    const unsigned vbits = (unsigned)(vw >> (32 * (wave & 1)));             // validity of this wave's 32 keys
                    if (tok0 < Tcur && (tok0 >> 6) < pg.max_pages) {
                        const int phys = pg.page_table[bb * pg.max_pages + (tok0 >> 6)];
                        const int64_t pe = pg.pool.page_elems();
                        _Float16* kpage = static_cast<_Float16*>(pg.pool.base) + pg.layer * pg.pool.layer_stride + ((int64_t)(phys * 2) * H + hh) * pe;
                        _Float16* vpage = kpage + (int64_t)H * pe;
                        const int slot0 = tok0 & 63;
                        const float4* sKs = lds + stage * STAGE;
                        const float4* sVs = sKs + KB * 8;
                        {   // K: lane -> (token lane & 31, d-group 2 i + (lane >> 5))
                            const int tk = lane & 31, key = wave * 32 + tk;
                            const bool ok = (vbits >> tk) & 1u;
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int j = 2 * i + (lane >> 5);
                                const float4 v = sKs[key * 8 + (j ^ (key & 7))];
                                if (ok) *reinterpret_cast<float4*>(kpage + ((int64_t)j * 64 + slot0 + tk) * 8) = v;
                            }
                        }
                        {   // V: lane -> (token 8 i + (lane >> 3), 16-byte chunk lane & 7): 1 KB of consecutive bytes per instruction
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int tk = 8 * i + (lane >> 3), key = wave * 32 + tk, ch = lane & 7;
                                const float4 v = sVs[key * 8 + (ch ^ (((key >> 1) & 3) << 1))];
                                if ((vbits >> tk) & 1u) *reinterpret_cast<float4*>(vpage + ((int64_t)(slot0 + tk) * 64 + ch * 8)) = v;
                            }
                        }
                    }
                }
            }
        }
        int nitem = item, nkbi = kb + 1;
        if (nkbi == nkb) { nitem = item + gridDim.x; nkbi = 0; }
        // PIPE, full stage: the next unit's 8 LDS-DMA pieces are issued inside the tile loop below, a quarter per tile, instead of as a
        // burst here (stamps, round 3: 0.85 us per unit during which all 8 waves only issue and the matrix pipe idles)
        const bool dma_in_loop = PIPE && NW == 8 && (kb + 1) * KB <= Tcur;
        const ItemBase nbase = item_base(nitem < n_items ? nitem : item);   // (two integer divisions: once per unit, not once per piece)
        if (nitem < n_items) {                                    // the other stage was last read before the barrier above
            if (!dma_in_loop) issue(nitem, nkbi, stage ^ 1);
            mk = mask_of(nitem, nkbi);
            if (nkbi == 0) load_q(nitem);
        }
        MGEA_FLUSH_OUT();
        optr = nullptr;
        PH_STAMP(un * 8 + 3);

        const float4* sK = lds + stage * STAGE;
        const bf16_t* sV = reinterpret_cast<const bf16_t*>(lds + stage * STAGE + KB * 8);
        // ---- one 64-key tile in three pieces (lambdas, so that the two loop forms below share them) ----
        // S^T = K Q^T of keys t0 .. t0 + 63 against the wave's 32 queries: two independent chains per key tile (both query blocks)
        auto qk_tile = [&](int t0, f32x4 (&sc)[2][4]) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) { sc[0][kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; sc[1][kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const int key = t0 + kt * 16 + c;
                    const float4 kv = sK[key * 8 + ((ks * 4 + g) ^ (key & 7))];
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&kv);
                    sc[0][kt] = X16<E>::mfma(kf, qf[0][ks], sc[0][kt]);
                    sc[1][kt] = X16<E>::mfma(kf, qf[1][ks], sc[1][kt]);
                }
        };
        // key mask, tile maximum, and the (rare) move of the scaling reference with its accumulator rescale
        auto tile_max = [&](int t0, f32x4 (&sc)[2][4], bool first_tile) {
            const unsigned long long vm = sValid[stage * VW + (t0 >> 6)];
            const unsigned vm_lo = __builtin_amdgcn_readfirstlane((unsigned)vm), vm_hi = __builtin_amdgcn_readfirstlane((unsigned)(vm >> 32));
            const bool all_valid = (vm_lo & vm_hi) == 0xffffffffu;                         // wave-uniform
            const unsigned vb_lo = vm_lo >> (4 * g), vb_hi = vm_hi >> (4 * g);              // bit 16 (kt & 1) + r of word kt >> 1
            float tmax[2];
#pragma unroll
            for (int mq = 0; mq < 2; ++mq) {
                tmax[mq] = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    if (!all_valid) {
                        const unsigned w = (kt >> 1) ? vb_hi : vb_lo;
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[mq][kt][r] = ((w >> (16 * (kt & 1) + r)) & 1u) ? sc[mq][kt][r] : -INFINITY;
                    }
                    const float m4 = max_nc(max_nc(sc[mq][kt][0], sc[mq][kt][1]), max_nc(sc[mq][kt][2], sc[mq][kt][3]));
                    tmax[mq] = kt == 0 ? m4 : max_nc(tmax[mq], m4);
                }
            }
            tmax[0] = quad_max(tmax[0]);
            tmax[1] = quad_max(tmax[1]);
            // Deferred rescale (guide T13): the running maximum is only a scaling reference; P and the accumulators stay exact as long
            // as one reference is used per row.  Keep the old one while no row of this wave outgrows it by more than 2^RESCALE_LOG2
            // (X16<E>::attn_rescale_log2, a property of the element type: P is stored as E, so 2^RESCALE_LOG2 must stay finite in E --
            // 2^16 for bf16, 2^15 for fp16, where 2^16 is +inf and made lacc inf and the output row NaN) -- the accumulator rescale and
            // its exponential then run on the first tile of an item and on the rare tile that trips the threshold instead of on every tile.
            constexpr float RESCALE_LOG2 = X16<E>::attn_rescale_log2;
            bool grow = first_tile;
            if (!first_tile) {
                const bool g0 = (tmax[0] - mx[0]) * kexp > RESCALE_LOG2, g1 = (tmax[1] - mx[1]) * kexp > RESCALE_LOG2;   // -inf - -inf = NaN: false
                grow = __any((g0 || g1) ? 1 : 0) != 0;                                                                  // wave-uniform
            }
            if (grow) {
#pragma unroll
                for (int mq = 0; mq < 2; ++mq) {
                    const float mnew = fmaxf(mx[mq], tmax[mq]);
                    if (!first_tile) {
                        // alpha = 2^((m_old - m_new) kexp); rows that had no valid key so far carry zeros: any finite alpha will do
                        const float alpha = (mx[mq] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mx[mq] - mnew) * kexp);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt) {
                            oacc[mq][dt][0] *= alpha; oacc[mq][dt][1] *= alpha; oacc[mq][dt][2] *= alpha; oacc[mq][dt][3] *= alpha;
                        }
                        lacc[mq][0] *= alpha; lacc[mq][1] *= alpha; lacc[mq][2] *= alpha; lacc[mq][3] *= alpha;
                    }
                    mx[mq] = mnew;
                }
            }
        };
        // P = 2^((s - m) kexp) as the 16-bit operand (straight from the accumulator registers), its row sums, and O += P V
        auto exp_half = [&](f32x4 (&sc)[2][4], bf16x8 (&pf)[2][2], int p) {
#pragma unroll
            for (int mq = 0; mq < 2; ++mq) {
                const float nml = (mx[mq] == -INFINITY) ? 0.f : -mx[mq] * kexp;   // a row without a valid key yet: p = 2^(-inf) = 0
#pragma unroll
                for (int kt = 2 * p; kt < 2 * p + 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        pf[mq][p][(kt & 1) * 4 + r] = (bf16_t)__builtin_amdgcn_exp2f(fmaf(sc[mq][kt][r], kexp, nml));
            }
        };
        auto pv_half = [&](int t0, bf16x8 (&pf)[2][2], int p) {
            lacc[0] = X16<E>::mfma(ones, pf[0][p], lacc[0]);      // row sums of the 16-bit P the P V product actually uses
            lacc[1] = X16<E>::mfma(ones, pf[1][p], lacc[1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16_t* vb = sV + (t0 + 32 * p) * 64 + v_off[dt];
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + 16 * 64));
                union { s16x4 s[2]; bf16x8 v; } u;
                u.s[0] = lo; u.s[1] = hi;
                oacc[0][dt] = X16<E>::mfma(u.v, pf[0][p], oacc[0][dt]);
                oacc[1][dt] = X16<E>::mfma(u.v, pf[1][p], oacc[1][dt]);
            }
        };
        if (PIPE && (kb + 1) * KB <= Tcur) {
            // SOFTWARE-PIPELINED form for a full stage (round 4).  In the rolled loop below a tile is Q K^T (16 MFMAs), then ~190 vector
            // instructions of softmax, then P V (20 MFMAs): matrix pipe and vector ALU take turns -- 576 + ~770 cycles per wave and
            // tile, and the two waves of a SIMD, which run the same program between the same barriers, do it in lockstep (2,600 cycles
            // per pair of tiles by in-kernel stamps, round 3: the SUM).  Here the stage's tiles are unrolled and the NEXT tile's
            // Q K^T is issued between this tile's maximum and its exponentials (scores double-buffered, +32 registers), and P V of the
            // first 32 keys runs under the exponentials of the other 32: the MFMAs of one tile sit in the shadow of the vector work of
            // its neighbours, inside ONE wave's instruction stream (hipcc interleaves what is independent within a basic block).
            constexpr int NT = KB / 64;
            f32x4 sc[2][2][4];
            qk_tile(0, sc[0]);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                tile_max(64 * i, sc[i & 1], kb == 0 && i == 0);
                if (dma_in_loop && nitem < n_items) issue_part(nbase, nkbi, stage ^ 1, i * 4 / NT, (i + 1) * 4 / NT);
                bf16x8 pf[2][2];
                if (i + 1 < NT) qk_tile(64 * (i + 1), sc[(i + 1) & 1]);
                exp_half(sc[i & 1], pf, 0);
                exp_half(sc[i & 1], pf, 1);
                pv_half(64 * i, pf, 0);
                pv_half(64 * i, pf, 1);
            }
        } else {
#pragma unroll 1
            for (int t0 = 0; t0 < KB && kb * KB + t0 < Tcur; t0 += 64) {   // workgroup-uniform bounds (packed input: this sequence's length)
                f32x4 sc[2][4];                                   // both query blocks side by side: two independent dependency chains per wave
                bf16x8 pf[2][2];                                  // [query block][32-key half]
                qk_tile(t0, sc);
                tile_max(t0, sc, kb == 0 && t0 == 0);
                exp_half(sc, pf, 0);
                exp_half(sc, pf, 1);
                pv_half(t0, pf, 0);
                pv_half(t0, pf, 1);
            }
        }

        PH_STAMP(un * 8 + 4);
        if (kb == nkb - 1) {
            const int bh = item / nqb, qb = item - bh * nqb, bb = bh / H, hh = bh - bb * H;
            __syncthreads();                                      // every wave is done with this stage's K image
            bf16_t* so = reinterpret_cast<bf16_t*>(lds + stage * STAGE) + wave * (32 * 64);   // [32 queries][64 d], chunk ^= query & 7
#pragma unroll
            for (int mq = 0; mq < 2; ++mq) {
                // 1 ulp, far below the bf16 output rounding; a row without ANY valid key (all-zero mask) has lacc == 0 and oacc == 0:
                // it gets zeros, not rcp(0) * 0 = NaN (the reference's finfo.min mask would attend uniformly to padding there --
                // an input the tokenizer never produces: [CLS] is always valid)
                const float inv = lacc[mq][0] > 0.f ? __builtin_amdgcn_rcpf(lacc[mq][0]) : 0.f;
                const int ql = mq * 16 + c;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    bf16x4 o = {(bf16_t)(oacc[mq][dt][0] * inv), (bf16_t)(oacc[mq][dt][1] * inv), (bf16_t)(oacc[mq][dt][2] * inv),
                                (bf16_t)(oacc[mq][dt][3] * inv)};
                    const int ch = (dt * 2 + (g >> 1)) ^ (ql & 7);
                    *reinterpret_cast<bf16x4*>(so + ql * 64 + ch * 8 + 4 * (g & 1)) = o;
                }
            }
            // a wave reads back only what it wrote itself: lane -> row (lane >> 3) + 8 i, 16-byte chunk lane & 7
            {
                const int ql = lane >> 3, ch = lane & 7;             // (8 i + ql) & 7 == ql
                const bf16_t* sp = so + ql * 64 + ((ch ^ ql) * 8);
                ov0 = *reinterpret_cast<const float4*>(sp);
                ov1 = *reinterpret_cast<const float4*>(sp + 8 * 64);
                ov2 = *reinterpret_cast<const float4*>(sp + 16 * 64);
                ov3 = *reinterpret_cast<const float4*>(sp + 24 * 64);
            }
            orow = qb * QPB + wave * 32 + (lane >> 3);
            oT = Tcur;
            optr = out + ((int64_t)row0cur + orow) * C + hh * DH + (lane & 7) * 8;
        }
        item = nitem; kb = nkbi; stage ^= 1;
        PH_STAMP(un * 8 + 5);
        ++un;
    }
    MGEA_FLUSH_OUT();
#undef MGEA_FLUSH_OUT
}

template <typename E, int NW, int PIPE>
static int launch_attn16(const void* qkv, const int32_t* mask, void* out, int B, int T, int H, hipStream_t st, const KvPages& pg, const int32_t* cu) {
    constexpr int QPB = 32 * NW, KB = 32 * NW;
    const int nqb = ceil_div(T, QPB);
    const int64_t n_items = (int64_t)B * H * nqb;
    MGEA_REQUIRE(n_items < (1 << 30), MGEA_EINVAL, "16-bit attention: too many (batch, head, query block) items");
    DeviceInfo di;
    MGEA_TRY(device_info(&di));
    const int shmem = 2 * KB * 16 * 16 + 64;
    static uint64_t attr_done = 0;                     // per instantiation
    MGEA_TRY(set_max_dynamic_lds((const void*)attn_bf16_kernel<E, NW, PIPE>, shmem, di.dev, &attr_done));
    const int per_cu = NW == 4 ? 2 : 1;
    const int grid = (int)(n_items < per_cu * di.n_cu ? n_items : per_cu * di.n_cu);
    hipLaunchKernelGGL((attn_bf16_kernel<E, NW, PIPE>), dim3(grid), dim3(64 * NW), shmem, st, (const E*)qkv, mask, (E*)out, T, H, (int)n_items, nqb,
                       0.125f, pg, cu);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}

int launch_attn_bf16(const void* qkv, const int32_t* mask, void* out, int B, int T, int H, int dh, hipStream_t st, int f16, const KvPages* pages,
                     const int32_t* cu) {
    MGEA_REQUIRE(dh == 64, MGEA_EINVAL, "bf16 attention: head_dim %d not supported (64)", dh);
    MGEA_REQUIRE(B > 0 && T > 0 && B <= 65535 && H <= 65535, MGEA_EINVAL, "bf16 attention: bad shape");
    MGEA_REQUIRE((int64_t)T * 6 * H * dh < ((int64_t)1 << 32), MGEA_EINVAL, "bf16 attention: one sequence of qkv rows must span < 4 GB");
    // long sequences: 256 queries / 256 keys per unit (switch attn16_wide: 0 never, 1 from 512 tokens (default), 2 always)
    const int wide = tune(TUNE_ATTN16_WIDE);
    bool w8 = wide == 2 || (wide == 1 && T >= 512);
    if (cu) {   // packed input: T = the longest sequence, which must fit one query block / key stage of the form that runs it
        MGEA_REQUIRE(!mask && T <= 256, MGEA_EINVAL, "16-bit attention over packed rows: no key mask, sequences of at most 256 tokens (got %d)", T);
        w8 = T > 128;
    }
    // the wide form runs its full stages software-pipelined (round 4; switch attn16_pipe = 0: the rolled tile loop).  The 4-wave form keeps
    // the rolled loop: at 128 keys it is memory-bound and the pipelined body spilled 31 registers (44 -> 54 us on [256, 128, 12 x 64])
    const bool pipe = tune(TUNE_ATTN16_PIPE) != 0;
    // (a static priority for waves 4..7 -- guide T5, static form -- on top of the pipelined body: 224.9 vs 227.0 us, nothing; not kept)
    const KvPages none{};
    const KvPages& pg = pages ? *pages : none;
    if (f16) {
        if (w8) return pipe ? launch_attn16<_Float16, 8, 1>(qkv, mask, out, B, T, H, st, pg, cu) : launch_attn16<_Float16, 8, 0>(qkv, mask, out, B, T, H, st, pg, cu);
        return launch_attn16<_Float16, 4, 0>(qkv, mask, out, B, T, H, st, pg, cu);
    }
    MGEA_REQUIRE(!pg.pool.base, MGEA_EINVAL, "16-bit attention: KV pages are written by the fp16 instantiation only");
    if (w8) return pipe ? launch_attn16<bf16_t, 8, 1>(qkv, mask, out, B, T, H, st, pg, cu) : launch_attn16<bf16_t, 8, 0>(qkv, mask, out, B, T, H, st, pg, cu);
    return launch_attn16<bf16_t, 4, 0>(qkv, mask, out, B, T, H, st, pg, cu);
}

}  // namespace mgea
