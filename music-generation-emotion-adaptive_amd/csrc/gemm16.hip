// The 16-bit GEMMs C[M, N] = epi(A[M, K] @ W[N, K]^T + bias) of the perf modes: bf16 for DistilBERT (BASELINE.json configs[1]: B = 256,
// S = 128), fp16 for the decoder's big-batch prefill.  16-bit storage, fp32 accumulation in the MFMAs, fp32 epilogue math; validated
// against the oracle on rounded weights (tests/test_gpu_bf16.py, tests/test_gpu_f16.py) and family by family on exact integer operands
// (tests/test_gpu_gemm16_plan.py).  Four kernel families, chosen by plan_gemm16 (gemm16_plan.h) and launched at the end of this file:
// * gemm_bf16_nt_kernel (G16_SMALL): v_mfma_f32_16x16x32_bf16, 128x128x64 tiles, 4 waves (2x2, 64x64 per wave), LDS tiles
//   [row][8 x 16 B] with the 16-B chunk XOR-swizzled by row&7 (conflict-free ds_write_b128 staging and ds_read_b128 fragments),
//   register-staged double buffering (next tile's global loads fly under this tile's MFMAs), XCD-aware tile order, "swapped" MFMA so
//   a lane owns 4 consecutive output columns (8-byte bf16 stores).
// * gemm_bf16_glds_kernel (G16_RING): operands HBM/L2 -> LDS by LDS-DMA, 128 x 128 / 256 x 128 / 256 x 256 tiles.
// * gemm_bf16_ph_kernel (G16_PERSISTENT): one workgroup per CU, phase-interleaved 256 x 256 tiles, the only one with the
//   folded-LayerNorm epilogues and fp16 operands; with the stamp / ablation macros of the tools build (tools/build_stamps.sh).
// * gemm16_duo_kernel (G16_DUO): two independent 256 x 128 workgroups per CU (switch bf16_gemm_tile = 5).
#include <stdlib.h>

#include "x16.h"

namespace mgea {

template <int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_nt_kernel(const bf16_t* __restrict__ A, int lda,
                                                          const bf16_t* __restrict__ W, int ldw,
                                                          const float* __restrict__ bias,
                                                          const bf16_t* __restrict__ res, bf16_t* __restrict__ C,
                                                          int ldc, int M, int N, int K, int tiles_n) {
    constexpr int BM = 128, BN = 128;
    __shared__ float4 lds[2][(BM + BN) * 8];  // 16-B chunks: [buf][row*8 + (chunk ^ (row&7))]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    int bid = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) bid = (bid & 7) * (nblk >> 3) + (bid >> 3);  // XCD-contiguous tile runs
    const int m0 = (bid / tiles_n) * BM, n0 = (bid % tiles_n) * BN;
    const int KT = K >> 6;

    f32x4 acc[4][4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float4 ra[4], rw[4];
    auto load_tile = [&](int kt) {
        const int k0 = kt * 64;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * 256, row = idx >> 3, ch = idx & 7;
            int r = m0 + row; r = r < M ? r : M - 1;
            ra[i] = *reinterpret_cast<const float4*>(A + (int64_t)r * lda + k0 + ch * 8);
            int q = n0 + row; q = q < N ? q : N - 1;
            rw[i] = *reinterpret_cast<const float4*>(W + (int64_t)q * ldw + k0 + ch * 8);
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * 256, row = idx >> 3, ch = idx & 7;
            lds[buf][row * 8 + (ch ^ (row & 7))] = ra[i];
            lds[buf][(BM + row) * 8 + (ch ^ (row & 7))] = rw[i];
        }
    };
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < KT; ++t) {
        const int buf = t & 1;
        if (t + 1 < KT) load_tile(t + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float4 v = lds[buf][(wm * 64 + m * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                af[m] = *reinterpret_cast<const bf16x8*>(&v);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const float4 v = lds[buf][(BM + wn * 64 + n * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                wf[n] = *reinterpret_cast<const bf16x8*>(&v);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], af[m], acc[n][m], 0, 0, 0);
        }
        if (t + 1 < KT) store_tile(buf ^ 1);
        __syncthreads();
    }
    // D[i = output column 4g + r][j = output row c]
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int row = m0 + wm * 64 + m * 16 + c;
        if (row >= M) continue;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = n0 + wn * 64 + n * 16 + 4 * g;
            if (col >= N) continue;
            float4 v = make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]);
            if (bias) v = add4(v, ld4(bias + col));
            if (EPI == BEPI_BIAS_GELU) v = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
            if (EPI == BEPI_BIAS_RES) {
                const bf16x4 r4 = *reinterpret_cast<const bf16x4*>(res + (int64_t)row * ldc + col);
                v = add4(v, make_float4((float)r4[0], (float)r4[1], (float)r4[2], (float)r4[3]));
            }
            bf16x4 o = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
            *reinterpret_cast<bf16x4*>(C + (int64_t)row * ldc + col) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Large-M variant: 256 x (64*NT) tile, 8 waves (2 x 4, 128 x 16*NT per wave), BK = 64, operands go
// HBM/L2 -> LDS directly with global_load_lds_dwordx4 (no staging registers, no ds_write pass).
// The LDS image is lane-linear per wave instruction (8 rows x 128 B), so the XOR swizzle is applied
// on the SOURCE address: the lane that fills LDS chunk (row, ch') fetches global chunk ch' ^ (row&7),
// and the fragment reads use the same involution.  Two LDS buffers: the loads of tile t+1 are issued
// before the MFMAs of tile t and drained (vmcnt(0)) just before the barrier that ends it.
// WMW = waves along M (each 128 rows): WMW = 2 -> 256-row tile, 8 waves, one workgroup per CU;
// WMW = 1 -> 128-row tile, 4 waves, 64 KB of LDS, two workgroups per CU whose barriers interleave.
template <int EPI, int NT, int WMW>
__global__ __launch_bounds__(256 * WMW) void gemm_bf16_glds_kernel(const bf16_t* __restrict__ A, int lda,
                                                            const bf16_t* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias,
                                                            const bf16_t* __restrict__ res, bf16_t* __restrict__ C,
                                                            int ldc, int M, int N, int K, int tiles_n) {
    constexpr int BM = 128 * WMW, BN = 64 * NT, NTHR = 256 * WMW;
    constexpr int WPW = (BN / 8) / (4 * WMW);           // W pieces (8 rows x 128 B) per wave per tile
    constexpr int SA = BM * 8, STAGE = (BM + BN) * 8;   // in 16-byte chunks
    extern __shared__ __attribute__((aligned(16))) float4 lds[];  // [2][STAGE]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;
    int bid = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) bid = (bid & 7) * (nblk >> 3) + (bid >> 3);
    const int m0 = (bid / tiles_n) * BM, n0 = (bid % tiles_n) * BN;
    const int KT = K >> 6;

    // per-lane source of the glds pieces: piece p covers rows 8p .. 8p+7; lane -> (row 8p + lane/8, chunk)
    const int lr = lane >> 3, lch = (lane & 7) ^ lr;
    const bf16_t* asrc[4];
    const bf16_t* wsrc[WPW];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = m0 + (wave * 4 + i) * 8 + lr;
        r = r < M ? r : M - 1;
        asrc[i] = A + (int64_t)r * lda + lch * 8;
    }
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
        int r = n0 + (wave * WPW + i) * 8 + lr;
        r = r < N ? r : N - 1;
        wsrc[i] = W + (int64_t)r * ldw + lch * 8;
    }
    auto issue = [&](int buf, int kt) {
        const int k0 = kt * 64;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + k0),
                                             (__attribute__((address_space(3))) void*)(lds + buf * STAGE + (wave * 4 + i) * 64),
                                             16, 0, 0);
#pragma unroll
        for (int i = 0; i < WPW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + k0),
                                             (__attribute__((address_space(3))) void*)(lds + buf * STAGE + SA + (wave * WPW + i) * 64),
                                             16, 0, 0);
    };

    f32x4 acc[NT][8];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // NS-deep LDS ring (3 stages of 48 KB for the 256x128 tile, 2 of 64 KB for 256x256): NS-1 tiles are
    // in flight while one is consumed.  Counted vmcnt + raw s_barrier: a __syncthreads() would drain
    // the LDS-DMA queue (vmcnt(0)) at every tile.  RAW: each wave waits for ITS pieces of tile t+1,
    // then the barrier makes all pieces visible before iteration t+1 reads them.  WAR: the buffer
    // re-filled in iteration t was last read in iteration t-1, behind that iteration's barrier.
    constexpr int NS = (NT == 2 && WMW == 2) ? 3 : 2;
    constexpr int PER_TILE = 4 + WPW;             // glds instructions per wave per tile
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < KT) issue(s, s);
    if (KT > NS - 2 && NS > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * PER_TILE) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int cur = 0, nxt = NS - 1;                     // ring slots of tile t and of tile t + NS - 1
    for (int t = 0; t < KT; ++t) {
        const float4* sb = lds + cur * STAGE;
        const bool more = t + NS - 1 < KT;
        if (more) issue(nxt, t + NS - 1);
        cur = cur + 1 == NS ? 0 : cur + 1;
        nxt = nxt + 1 == NS ? 0 : nxt + 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 wf[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float4 v = sb[SA + (wn * 16 * NT + n * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                wf[n] = *reinterpret_cast<const bf16x8*>(&v);
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const float4 v = sb[(wm * 128 + m * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(&v);
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], af, acc[n][m], 0, 0, 0);
            }
        }
        // tile t+1 must have landed; the tiles issued after it (NS-2 of them) may stay in flight
        if (more && NS > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * PER_TILE) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    // Epilogue through LDS (the operand ring is free now): the MFMA layout gives each lane 4 columns
    // of one row (8-byte pieces, 16 rows per instruction); staged as a [256][BN] bf16 tile and
    // streamed out as whole rows, 16 bytes per lane -> full-line stores and residual reads.
    constexpr int PITCH = BN * 2 + 16;            // bytes; +16 keeps 16-B alignment and staggers banks
    unsigned char* sC = reinterpret_cast<unsigned char*>(lds);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                 // every wave is done reading the last operand tile
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int lrow = wm * 128 + m * 16 + c;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int lcol = wn * 16 * NT + n * 16 + 4 * g;
            float4 v = make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]);
            if (bias && n0 + lcol < N) v = add4(v, ld4(bias + n0 + lcol));
            if (EPI == BEPI_BIAS_GELU) v = make_float4(gelu_fast(v.x), gelu_fast(v.y), gelu_fast(v.z), gelu_fast(v.w));
            bf16x4 o = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
            *reinterpret_cast<bf16x4*>(sC + lrow * PITCH + lcol * 2) = o;
        }
    }
    __syncthreads();
    constexpr int CPR = BN / 8;                   // 16-byte chunks per tile row
#pragma unroll
    for (int i = 0; i < BM * CPR / NTHR; ++i) {
        const int id = tid + i * NTHR, lrow = id / CPR, ch = id % CPR;
        const int row = m0 + lrow, col = n0 + ch * 8;
        if (row < M && col < N) {
            bf16x8 v = *reinterpret_cast<const bf16x8*>(sC + lrow * PITCH + ch * 16);
            if (EPI == BEPI_BIAS_RES) {
                const bf16x8 r8 = *reinterpret_cast<const bf16x8*>(res + (int64_t)row * ldc + col);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (bf16_t)((float)v[j] + (float)r8[j]);
            }
            *reinterpret_cast<bf16x8*>(C + (int64_t)row * ldc + col) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------
// 256 x 256 x 64 tile, 8 waves (2 along M x 4 along N, 128 x 64 of C per wave), the phase-interleaved structure of the
// CDNA4 GEMM playbook (cdna_hip_programming.md T3+T4, "The 256^2 8-phase template"), written out from its rules:
//
//   * a K-tile is consumed in 4 PHASES of 16 MFMAs (one 64 x 32 quadrant of the wave's C over the whole BK = 64).  A phase is
//     [L-segment: ds_read the fragments this phase's MFMAs need, issue 2 global_load_lds (this wave's share of one
//      128-row half-tile of a LATER K-tile), wait for the reads] s_barrier [C-segment: 16 MFMAs] s_barrier.
//   * waves 4-7 (the second wave of every SIMD) run ONE BARRIER LATER than waves 0-3: in every barrier-to-barrier interval
//     one wave of each SIMD is in its C-segment (matrix pipe) and the other in its L-segment (LDS + address VALU + DMA
//     issue) -- instead of both reading, then both fighting for the matrix pipe.
//   * operands go HBM/L2 -> LDS by LDS-DMA (no staging registers, no ds_write), two 64 KB stages; the loads of a tile are
//     issued 4-6 phases before its first read and are waited for with a COUNTED vmcnt once per K-tile (6 younger DMAs stay
//     in flight across it); raw s_barrier only (a __syncthreads() would drain the DMA queue).
//
// Hazards, by construction (u = K-tile, stage = u & 1, phases q = 4u + p; L(q) / C(q) of waves 0-3 are intervals 2q / 2q+1,
// of waves 4-7 intervals 2q+1 / 2q+2):
//   reads  : p0 reads B(j=0) + A(i=0), p1 B(j=1), p2 A(i=1), p3 nothing (B(j=0) stays in registers); every ds_read is
//            complete (lgkmcnt(0)) before the barrier that ends its L-segment.  So tile u's B halves are last read in
//            interval 2(4u+1)+1 and its A halves in interval 2(4u+2)+1.
//   WAR    : stage u & 1 is refilled with tile u+2: B-half 0 issued in phase 4u+2 (first interval 2(4u+2) > 2(4u+1)+1),
//            BOTH A halves in phase 4u+3 (2(4u+3) > 2(4u+2)+1), B-half 1 in phase 4(u+1).
//            (Round 2 issued A-half 1 in phase 4(u+1)+1, three phases before its first read: A is the operand that misses L2 -- an
//            A panel is shared by N / 256 tiles only, the W panel by every row tile of the XCD's run -- and in-kernel stamps
//            (tools/gemm_bf16_stamps.py) showed the K loop of the N = 768 GEMMs at 2.0 us per K-tile against 1.45 at N >= 2304.
//            The A halves now have the longest lookahead, 5 phases, the L2-resident B-half 1 the shortest, 4.)
//   RAW    : tile u+1 is first read in interval 2*4(u+1) = 8u+8.  Its last DMA (B-half 1) is issued in phase 4u; every wave
//            waits until ITS DMAs of tile u+1 have landed -- vmcnt(6): only the three half-tiles issued in phases 4u+2, 4u+3
//            may still be in flight -- at the end of interval 8u+7 (waves 0-3: end of C(4u+3); waves 4-7: end of L(4u+3)),
//            and the barrier that ends that interval publishes them to every wave.

// In-kernel time stamps of the persistent GEMM (cdna_hip_programming.md section 7), compiled ONLY into the tools build
// (tools/build_stamps.sh: -DMGEA_PH_STAMPS, a separate .so that tools/gemm_bf16_stamps.py loads); the product library has none of it.
#ifdef MGEA_PH_STAMPS
__device__ unsigned long long* g_ph_stamps = nullptr;      // [workgroup][64] 100 MHz ticks, written by thread 0
__device__ unsigned long long* g_ph_cycles = nullptr;      // same slots, shader-clock cycles (s_memtime): cycles / ticks = the clock the loop held
#define PH_STAMP(i) do { if (g_ph_stamps && tid == 0 && (i) < 64) { g_ph_stamps[(size_t)blockIdx.x * 64 + (i)] = __builtin_amdgcn_s_memrealtime(); \
                                                                    if (g_ph_cycles) g_ph_cycles[(size_t)blockIdx.x * 64 + (i)] = __builtin_amdgcn_s_memtime(); } } while (0)
extern "C" int mgea_dbg_set_ph_stamps(unsigned long long* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ph_stamps), &p, sizeof(p)); }
extern "C" int mgea_dbg_set_ph_cycles(unsigned long long* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ph_cycles), &p, sizeof(p)); }
// ablation (wrong results, tools-only build): every unit loads tile 0's operands -- 192 KB of A and W that never leave L2 -- to
// tell a K loop bound by operand DELIVERY (it speeds up) from one bound by instruction issue (it does not)
__device__ int g_ph_same_tile = 0;
extern "C" int mgea_dbg_set_ph_same_tile(int v) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ph_same_tile), &v, sizeof(v)); }
#define PH_TILE_FOR_LOADS(t) (g_ph_same_tile ? 0 : (t))
// more timing ablations of the whole-tile K loop (wrong results), chosen at COMPILE time (-DMGEA_PH_ABLATE=bits: a run-time test around
// the reads or the MFMAs changes the loop it is meant to measure -- it tripled it): bit 0 no LDS-DMA after the prologue, bit 1 no fragment
// reads, bit 2 no MFMAs
#ifndef MGEA_PH_ABLATE
#define MGEA_PH_ABLATE 0
#endif
#define PH_ABLATE_INIT
#define PH_ABLATE(bit) (((MGEA_PH_ABLATE) >> (bit)) & 1)
#else
#define PH_ABLATE_INIT
#define PH_ABLATE(bit) 0
#define PH_STAMP(i) do { } while (0)
#define PH_TILE_FOR_LOADS(t) (t)
#endif

template <int EPI, typename T, int PH>
__global__ __launch_bounds__(512) void gemm_bf16_ph_kernel(const T* __restrict__ A, int lda, const T* __restrict__ W, int ldw,
                                                          const float* __restrict__ bias, const T* __restrict__ res,
                                                          T* __restrict__ C, int ldc, int M, int N, int K, int tiles_n, int n_tiles,
                                                          int tail_mode, BfEpiLn ln) {
    typedef typename X16<T>::v8 v8;
    typedef typename X16<T>::v4 v4;
    typedef typename X16<T>::v2 v2;
    constexpr int BM = 256, BN = 256;
    constexpr bool LNF = EPI == BEPI_LNFOLD || EPI == BEPI_LNFOLD_GELU;
    constexpr bool RESV = EPI == BEPI_BIAS_RES || EPI == BEPI_RES_LN;
    constexpr int SA = BM * 8, STAGE = (BM + BN) * 8;     // in 16-byte chunks: A tile, then the W tile
    constexpr int CST = 2 * STAGE;                         // the epilogue's own 32 KB behind the two operand stages
    extern __shared__ __attribute__((aligned(16))) float4 lds[];   // [2][STAGE] + [2048] = 160 KB; all LDS in this one array
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int wm = wave >> 2, wn = wave & 3;               // wm = 1: the late group
    const int KT = K >> 6;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float4*)lds;   // LDS byte address of the ring
    PH_ABLATE_INIT

    // PERSISTENT: one workgroup per CU walks its output tiles.  Workgroups b and b + 8 share an XCD (round-robin dispatch, speed
    // only): XCD r = b % 8 gets the contiguous run of tiles [r * n_tiles / 8, (r + 1) * n_tiles / 8) so that the tiles in flight on
    // one L2 share A and W panels; the run is walked by the XCD's workgroups with stride gridDim.x / 8.
    const int wg_x = gridDim.x >> 3;                         // host: gridDim.x % 8 == 0
    const int slot = (int)blockIdx.x >> 3;
    const int run0 = ((int)blockIdx.x & 7) * ((n_tiles + 7) >> 3);
    const int per_x = (run0 + ((n_tiles + 7) >> 3) < n_tiles ? ((n_tiles + 7) >> 3) : n_tiles - run0);   // tiles in this XCD's run (<= 0: none)
    // HALF-TILE TAIL: 384 tiles on 256 workgroups are one full round and a half-empty one.  When the tiles left over after the full
    // rounds number at most half the XCD's workgroups, each of them is cut into two 128-row halves computed by two workgroups
    // INDEPENDENTLY (no exchange, no scratch, no co-residency assumption -- round 2 cut K instead and swapped fp32 partial sums
    // through a coherent scratch, which two such launches sharing the GPU could deadlock on): a half unit keeps the 256-wide W tile
    // and the whole K loop, its 8 waves own 64 x 64 of C each, in a K loop of its own (3 LDS stages of 48 KB, 2 phases per K-tile:
    // "HALF UNITS" below).  Every output element sees the same MFMA sequence over K as in a whole tile: the two schedules are
    // bitwise identical.  tail_mode 2 additionally lets the odd slots run their half unit FIRST, so that the two halves of the chip
    // reach their store bursts half a tile apart.
    const int full_rounds = per_x > 0 ? per_x / wg_x : 0, rem = per_x > 0 ? per_x - full_rounds * wg_x : 0;
    const bool split = (tail_mode & 3) != 0 && rem > 0 && 2 * rem <= wg_x;
    int u_tile = 0, u_mode = 0;                              // mode 0: whole tile, 1 / 2: rows 0..127 / 128..255 of a shared tile
    // (tail_mode bit 2 = walk the XCD's run of tiles from its END: a GEMM whose A operand is the previous kernel's output and larger
    // than what the 256 MB Infinity Cache keeps of it -- DistilBERT's FC2 reads FC1's 201 MB -- otherwise reads that operand in the
    // order it was written, the one order in which an LRU cache that has just lost the head of the stream misses on every line)
    const bool rev = (tail_mode & 4) != 0;
    auto run_tile = [&](int idx) { return run0 + (rev ? per_x - 1 - idx : idx); };
    // A lower half (mode 2: rows 128..255 of its tile) that starts at or beyond row M does not exist: with M % 256 in (0, 128] the
    // last row tile has no second half, and its set_tile() clamp `M - 1 - lm0` would be negative -- as an unsigned LDS-DMA offset
    // 4 GB past the end of A (found by reading; e.g. DistilBERT at B = 255, S = 128).  Such a workgroup has no tail unit.
    const bool my_half = split && slot < 2 * rem &&
                         !((slot & 1) && (run_tile(full_rounds * wg_x + (slot >> 1)) / tiles_n) * BM + 128 >= M);
    const bool half_first = my_half && (tail_mode & 3) == 2 && (slot & 1);
    auto get_unit = [&](int ui) -> bool {                   // the ui-th unit of this workgroup
        if (half_first) {                                    // the tail unit comes first, the whole tiles after it
            if (ui == 0) { u_tile = run_tile(full_rounds * wg_x + (slot >> 1)); u_mode = 1 + (slot & 1); return true; }
            ui -= 1;
            if (ui < full_rounds) { u_tile = run_tile(slot + ui * wg_x); u_mode = 0; return true; }
            return false;
        }
        if (ui < full_rounds) { u_tile = run_tile(slot + ui * wg_x); u_mode = 0; return true; }
        if (ui > full_rounds) return false;
        if (split) {
            if (!my_half) return false;
            u_tile = run_tile(full_rounds * wg_x + (slot >> 1));
            u_mode = 1 + (slot & 1);
            return true;
        }
        if (slot >= rem) return false;
        u_tile = run_tile(full_rounds * wg_x + slot); u_mode = 0;
        return true;
    };

    // LDS-DMA sources: a half-tile = 128 rows x 128 B = 16 pieces of 8 rows; wave w moves pieces 2w, 2w+1 of every half-tile.
    // The LDS image is lane-linear, so the XOR swizzle sits on the SOURCE chunk (lane -> row lane/8, chunk (lane%8) ^ (row%8)).
    const int lr = lane >> 3, lch = (lane & 7) ^ lr;
    // A piece's source = a wave-uniform 64-bit base in SGPRs (the unit's first A / W row, advanced by 128 bytes per K-tile with scalar
    // adds) + a 32-bit byte offset per lane (row inside the unit, clamped to the matrix, and the swizzled chunk): no vector
    // arithmetic per piece.  (Round 2 kept 8 full pointers per lane and added kt * 128 to one for every piece: two 64-bit VALU adds
    // per piece in the L-segments, whose instruction count is what the K loop is bound by -- beside the partner wave's MFMAs an
    // L-segment gets about one issue slot per MFMA.)
    unsigned voff[4][2];     // [half-tile: A0, A1, W0, W1][piece]
    const char *abase = nullptr, *wbase = nullptr;
    int m0 = 0, n0 = 0;
    auto set_tile = [&](int t, int md) {                    // md != 0: the 128 rows of that half sit in rows 0..127 of the A stage
        m0 = (t / tiles_n) * BM + (md == 2 ? 128 : 0); n0 = (t % tiles_n) * BN;
        const int lt = PH_TILE_FOR_LOADS(t), lm0 = (lt / tiles_n) * BM + (md == 2 ? 128 : 0), ln0 = (lt % tiles_n) * BN;   // (= m0, n0 in the product build)
        abase = reinterpret_cast<const char*>(A + (int64_t)lm0 * lda);
        wbase = reinterpret_cast<const char*>(W + (int64_t)ln0 * ldw);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int ra = hf * 128 + (wave * 2 + i) * 8 + lr;          // row inside the unit; the unit's first row is inside the matrix
                ra = lm0 + ra < M ? ra : M - 1 - lm0;
                voff[hf][i] = (unsigned)(ra * lda + lch * 8) * 2u;
                int rw = hf * 128 + (wave * 2 + i) * 8 + lr;
                rw = ln0 + rw < N ? rw : N - 1 - ln0;
                voff[2 + hf][i] = (unsigned)(rw * ldw + lch * 8) * 2u;
            }
    };
    auto issue_half = [&](int hid, int kt, int stage) {   // hid: 0 A rows 0..127, 1 A rows 128..255, 2 W rows 0..127, 3 W rows 128..255
        const char* base = (hid >= 2 ? wbase : abase) + kt * 128;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row0 = (hid & 1) * 128 + (wave * 2 + i) * 8;
            const unsigned dst = lds_base + (unsigned)(stage * STAGE + (hid >= 2 ? SA : 0) + row0 * 8) * 16u;
            glds16_hidden_s(base, voff[hid][i], dst);
        }
    };
    // HALF UNITS (128 x 256 of C, mode 1 / 2) have their own K loop: a K-tile is A 128 rows (16 KB) + W 256 rows (32 KB) = 48 KB, so
    // THREE stages fit where the whole tiles have two (stage 2 = bytes 96 K .. 144 K overlaps the epilogue's C stage, which is only
    // live between two K loops), and a K-tile is consumed in TWO phases of 16 MFMAs per wave (each wave owns 64 x 64 of C: quadrants
    // (0, 0) and (0, 1) of the whole-tile wave tile) -- half the barriers of the 4-phase loop, which with two of its phases empty
    // took 0.82 of a whole tile's time for half the work.  Schedule (phase q = 2u + p of K-tile u, stage u % 3; early / late wave
    // groups as above: L(q) / C(q) = intervals 2q / 2q+1 resp. 2q+1 / 2q+2):
    //   reads : p0 reads W(j=0) + A, p1 reads W(j=1); every ds_read complete (lgkmcnt(0)) before the barrier that ends its L-segment,
    //           so stage u % 3 is last read in interval 2(2u+1)+1 = 4u+3.
    //   WAR   : stage (u+3) % 3 = u % 3 is refilled with K-tile u+3 in phases 2(u+1) (A0) and 2(u+1)+1 (W0, W1), first interval
    //           2(2u+2) = 4u+4 > 4u+3.
    //   RAW   : K-tile u+1 is first read in interval 2*2(u+1) = 4u+4; all its DMAs were issued in phases 2u-2, 2u-1 (or the
    //           prologue); every wave waits for ITS pieces at the end of interval 4u+3 (early: end of C(2u+1), late: end of
    //           L(2u+1)) with vmcnt(6) -- only the 6 DMAs of K-tile u+2, issued in phases 2u and 2u+1, may still be in flight --
    //           and the barrier that ends that interval publishes them.
    constexpr int HSA = 128 * 8, HSTAGE = (128 + 256) * 8;   // half units: 16-byte chunks of the A part / of a stage
    auto issue_h = [&](int hid, int kt, int st3) {          // hid 0: A rows 0..127, 2 / 3: W rows 0..127 / 128..255
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row0 = (hid & 1) * 128 + (wave * 2 + i) * 8;
            const unsigned dst = lds_base + (unsigned)(st3 * HSTAGE + (hid >= 2 ? HSA : 0) + row0 * 8) * 16u;
            glds16_hidden_s((hid >= 2 ? wbase : abase) + kt * 128, voff[hid][i], dst);
        }
    };
    // whole tiles: tile 0 whole, then W0 / A0 / A1 of tile 1 (the steady state issues W0 and A0 + A1 of K-tile u+2 in phases 4u+2
    // and 4u+3, W1 of K-tile u+1 in phase 4u); half units: K-tiles 0 and 1 whole (6 + 6 DMAs per wave)
    auto issue_prologue = [&](int nkt, int md) {
        if (md == 0) {
            issue_half(2, 0, 0); issue_half(0, 0, 0); issue_half(3, 0, 0); issue_half(1, 0, 0);
            if (nkt > 1) {
                if (PH == 2)      { issue_half(2, 1, 1); issue_half(3, 1, 1); }                   // two-phase loop: W of K-tile 1
                else if (PH == 1) { issue_half(0, 1, 1); issue_half(1, 1, 1); }                   // pipelined loop: A of K-tile 1
                else              { issue_half(2, 1, 1); issue_half(0, 1, 1); issue_half(1, 1, 1); }
            }
        } else {
            issue_h(2, 0, 0); issue_h(0, 0, 0); issue_h(3, 0, 0);
            if (nkt > 1) { issue_h(2, 1, 1); issue_h(0, 1, 1); issue_h(3, 1, 1); }
        }
    };

    // STREAM ACROSS WHOLE TILES: when this unit and the next are both whole tiles, the LDS-DMA schedule simply continues over the
    // boundary -- the "K-tile u+1 / u+2" of the last two K-tiles are the next unit's K-tiles 0 / 1 (their source addresses replace this
    // unit's in phase 1 of K-tile nkt-2, after this unit's last DMA and before the next unit's first) -- instead of a burst of 14 DMAs
    // per wave between the K loop and the epilogue (stamps: 1.7 us per tile during which all 8 waves only issue, and K-tile 0 / 1 get
    // half the lookahead).  Stages keep alternating: the next unit reads K-tile v from stage (v + sb) & 1, sb = (sb + nkt) & 1.
    // The hazard analysis above is unchanged: it is the same schedule with tile indices taken modulo the unit.  Units next to a half
    // unit (other stage geometry) and single-K-tile units start from the burst as before, with sb = 0.
    int ui = 0, sb = 0;
    bool streamed_in = false;                               // this unit's first K-tiles were issued inside the previous unit's K loop
    bool have = get_unit(0);
    int cur_tile = u_tile, cur_mode = u_mode;
    if (have) { set_tile(cur_tile, cur_mode); issue_prologue(KT, cur_mode); }
    while (have) {
        const int cm0 = m0, cn0 = n0;                       // this unit's origin (set_tile moves on to the next one below)
        const int nkt = KT, mode = cur_mode;
        const bool nx_have = get_unit(ui + 1);              // peek: u_tile / u_mode now describe the NEXT unit
        const int nx_tile = u_tile, nx_mode = u_mode;
        const bool stream = nx_have && nx_mode == 0 && mode == 0 && nkt >= 2;
        const int sbase = ui * 12;
        PH_STAMP(sbase + 0);                                // unit start
        const bool halfu = mode != 0;                       // workgroup-uniform
        const int wrows = halfu ? 64 : 128;                 // rows of the unit per wave row wm
        f32x4 acc[4][8];             // [n-tile of 16 columns][m-tile of 16 rows]
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // K-tile 0 has landed when at most the 6 DMAs of K-tile 1 issued by the prologue (W0 / A0 / A1 of a whole tile, all of a half
        // unit's) are still in flight.  (After the first unit the previous epilogue's stores are younger than these DMAs and count too: the
        // wait is then stronger, never weaker.)
        // (pipelined loop, unit streamed into: the previous unit's last barrier has already published this unit's K-tile 0)
        if (!(PH == 1 && streamed_in)) {
        if (nkt > 1) {
            if (PH != 4 && !halfu) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else               asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (wm == 1 && (PH != 1 || halfu)) __builtin_amdgcn_s_barrier();   // the late group starts one interval later (phase loops)
        }
        PH_STAMP(sbase + 1);                                // K-tile 0 landed, K loop starts

        v8 af[4][2], bf0[2][2], bf1[2][2];                // A: 4 m-tiles x 2 k-steps; W: 2 n-tiles x 2 k-steps, for j = 0 and j = 1
        if (!halfu && PH == 1) {
        // SOFTWARE-PIPELINED loop, ONE barrier per K-tile (switch bf16_gemm_phases = 1).  The phase loops separate a wave's LDS reads /
        // DMA issue (L-segment) from its MFMAs (C-segment) with a barrier and run the two waves of a SIMD in opposite roles; the
        // stamps and ablations of round 3 say what that costs: a K-tile's 64 MFMAs per wave are 1.0 us of matrix pipe for the SIMD's
        // two waves, the barrier skeleton alone (8 intervals) 0.69 us, the loop 1.5-1.6 us -- an interval is as long as the LONGER of
        // one wave's L-segment and the other's C-segment plus a barrier turn-around.  Here every wave runs ONE stream per K-tile: four
        // quarters of 16 MFMAs (quarter (ks, i): k-step ks of the K-tile, 64-row half i of the wave's rows, all 4 n-tiles), and among
        // the MFMAs of a quarter it reads the NEXT quarter's fragments into the other half of a double buffer (fa0 / fa1, fw0 / fw1:
        // the same 64 fragment registers as the phase loops) and issues its LDS-DMA pieces; hipcc counts lgkmcnt for the fragment
        // reads itself (it sees them), the DMAs stay hidden and hand-counted.  Nothing separates the two waves of a SIMD: the hardware
        // issues one wave's MFMAs under the other's reads and DMA issue.
        //   q0 (ks0, i0): reads A(ks0, i1);              issues W0, W1 of K-tile u+1 (4 pieces per wave)
        //   q1 (ks0, i1): reads A(ks1, i0) and W(ks1)
        //   q2 (ks1, i0): reads A(ks1, i1);              then lgkmcnt(0), vmcnt(0), BARRIER
        //   q3 (ks1, i1): reads A(ks0, i0), W(ks0) of K-tile u+1 (other stage);   issues A0, A1 of K-tile u+2 (4 pieces)
        //   WAR : the stage of K-tile u is last read in q2 (complete before the barrier: lgkmcnt(0)); its refill (A of K-tile u+2 in
        //         q3 of K-tile u, W of K-tile u+2 in q0 of K-tile u+1) is issued after that barrier.
        //   RAW : K-tile u+1 (A issued in q3 of K-tile u-1, W in q0 of K-tile u; nothing younger) is first read in q3 of K-tile u; every
        //         wave waits for ITS pieces with vmcnt(0) at the end of q2 and the barrier publishes them.  A has a whole K-tile of
        //         lookahead, the L2-resident W three quarters.
        // Unit start: K-tile 0 landed and published, A of K-tile 1 in flight (prologue: K-tile 0 + A of K-tile 1; streamed into: the
        // same state, left by the previous unit's last two K-tiles); the unit's first fragments are read outside the pipeline.
        v8 fa0[4], fa1[4], fw0[4], fw1[4];
        auto rdA = [&](const float4* sa_, int i, int ks, int m) -> v8 {
            const float4 v = sa_[((i * 4 + m) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
            return *reinterpret_cast<const v8*>(&v);
        };
        auto rdW = [&](const float4* sw_, int ks, int n) -> v8 {
            const float4 v = sw_[(n * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
            return *reinterpret_cast<const v8*>(&v);
        };
        auto issue_piece = [&](int hid, int i, int kt, int stage) {   // one 1 KiB piece of half-tile hid (issue_half = pieces 0 and 1)
            const int row0 = (hid & 1) * 128 + (wave * 2 + i) * 8;
            const unsigned dst = lds_base + (unsigned)(stage * STAGE + (hid >= 2 ? SA : 0) + row0 * 8) * 16u;
            glds16_hidden_s((hid >= 2 ? wbase : abase) + kt * 128, voff[hid][i], dst);
        };
        {
            const float4* sbuf = lds + (sb & 1) * STAGE;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                fa0[m] = rdA(sbuf + (wm * 128) * 8, 0, 0, m);
                fw0[m] = rdW(sbuf + SA + (wn * 64) * 8, 0, m);
            }
        }
        if (PH_ABLATE(1)) {                                   // (tools-only ablation without fragment reads: defined, opaque operands)
#pragma unroll
            for (int m = 0; m < 4; ++m) { fa1[m] = fa0[m]; fw1[m] = fw0[m]; asm volatile("" : "+v"(fa1[m]), "+v"(fw1[m])); }
        }
        for (int u = 0; u < nkt; ++u) {
            const float4* sbuf = lds + ((u + sb) & 1) * STAGE;
            const float4* sa = sbuf + (wm * 128) * 8;
            const float4* sw = sbuf + SA + (wn * 64) * 8;
            const float4* nbuf = lds + ((u + 1 + sb) & 1) * STAGE;
            const float4* nsa = nbuf + (wm * 128) * 8;
            const float4* nsw = nbuf + SA + (wn * 64) * 8;
            const int g1 = u + 1, g2 = u + 2;               // K-tiles the DMAs of this K-tile belong to (>= nkt: the next unit's)
            const bool i1 = g1 < nkt || stream, i2 = g2 < nkt || stream;
            const int k1 = g1 < nkt ? g1 : g1 - nkt, k2 = g2 < nkt ? g2 : g2 - nkt;
            const bool nxt = g1 < nkt;
            // (reads come BEFORE the MFMAs of their group and in the first groups of a quarter, W fragments first: the next quarter's
            // first group needs all four W fragments and A fragment 0, and nothing is waited for right after it was requested)
            // ---------------- q0
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!PH_ABLATE(1)) fa1[m] = rdA(sa, 1, 0, m);
                if (i1 && !PH_ABLATE(0)) issue_piece(2 + (m >> 1), m & 1, k1, (g1 + sb) & 1);
#pragma unroll
                for (int n = 0; n < 4; ++n) if (!PH_ABLATE(2)) acc[n][m] = X16<T>::mfma(fw0[n], fa0[m], acc[n][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---------------- q1
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!PH_ABLATE(1)) {
                if (m == 0) { fw1[0] = rdW(sw, 1, 0); fw1[1] = rdW(sw, 1, 1); fw1[2] = rdW(sw, 1, 2); }
                if (m == 1) { fw1[3] = rdW(sw, 1, 3); fa0[0] = rdA(sa, 0, 1, 0); fa0[1] = rdA(sa, 0, 1, 1); }
                if (m == 2) { fa0[2] = rdA(sa, 0, 1, 2); fa0[3] = rdA(sa, 0, 1, 3); }
                }
#pragma unroll
                for (int n = 0; n < 4; ++n) if (!PH_ABLATE(2)) acc[n][4 + m] = X16<T>::mfma(fw0[n], fa1[m], acc[n][4 + m]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (stream && u == nkt - 2) {                     // this unit's last DMA is out (q0): the next unit's addresses
                int t = nx_tile;
                asm volatile("" : "+s"(t));                   // (opaque: hipcc otherwise computes the next unit's 8 offsets at the unit start and keeps them live)
                set_tile(t, 0);
            }
            // ---------------- q2
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (m < 2 && !PH_ABLATE(1)) { fa1[2 * m] = rdA(sa, 1, 1, 2 * m); fa1[2 * m + 1] = rdA(sa, 1, 1, 2 * m + 1); }
#pragma unroll
                for (int n = 0; n < 4; ++n) if (!PH_ABLATE(2)) acc[n][m] = X16<T>::mfma(fw1[n], fa0[m], acc[n][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every read of this stage is in registers before anyone may refill it
            if (i1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of K-tile u+1 have landed
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // ---------------- q3
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (nxt && !PH_ABLATE(1)) {
                    if (m == 0) { fw0[0] = rdW(nsw, 0, 0); fw0[1] = rdW(nsw, 0, 1); fw0[2] = rdW(nsw, 0, 2); }
                    if (m == 1) { fw0[3] = rdW(nsw, 0, 3); fa0[0] = rdA(nsa, 0, 0, 0); fa0[1] = rdA(nsa, 0, 0, 1); }
                    if (m == 2) { fa0[2] = rdA(nsa, 0, 0, 2); fa0[3] = rdA(nsa, 0, 0, 3); }
                }
                if (i2 && !PH_ABLATE(0)) issue_piece(m >> 1, m & 1, k2, (g2 + sb) & 1);
#pragma unroll
                for (int n = 0; n < 4; ++n) if (!PH_ABLATE(2)) acc[n][4 + m] = X16<T>::mfma(fw1[n], fa1[m], acc[n][4 + m]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        } else if (!halfu && PH == 2) {
        // TWO phases of 32 MFMAs per K-tile (switch bf16_gemm_phases = 2).  Compile-time ablations of the four-phase loop
        // (tools/gemm_bf16_ablate.sh) put the skeleton of a K-tile -- 8 barrier-to-barrier intervals with their reads and DMAs but
        // no MFMA -- at 0.89 us and its 64 MFMAs per wave at 1.0 us of matrix pipe for the SIMD's two waves, yet the loop takes 1.6 us:
        // every interval pays ~130 cycles of barrier turn-around on top of its 256 MFMA cycles.  Here a K-tile has 4 intervals of 512:
        //   reads : P0 reads W(j=0), W(j=1) and A(i=0) (16 ds_read_b128), P1 reads A(i=1) (8); the W fragments stay in registers.
        //           W of stage u & 1 is last read in interval 2(2u)+1 = 4u+1, A in interval 2(2u+1)+1 = 4u+3.
        //   WAR   : W0 / W1 of K-tile u+2 (same stage) are issued in phase 2u+1 (first interval 4u+2 > 4u+1), A0 / A1 of K-tile u+1
        //           (stage (u+1) & 1, last read in interval 4(u-1)+3 = 4u-1) in phase 2u (first interval 4u).
        //   RAW   : K-tile u+1 is first read in interval 4u+4; its W was issued in phase 2u-1, its A in phase 2u; every wave waits
        //           for ITS pieces at the end of interval 4u+3 (early: end of C(2u+1), late: end of L(2u+1)) with vmcnt(4) -- only
        //           the two W halves of K-tile u+2, issued in phase 2u+1, may still be in flight.
        // A gets 4 intervals (~2500 cycles) of lookahead instead of 10 x 390; W, the L2-resident operand, 6.
        for (int u = 0; u < nkt; ++u) {
            const float4* sbuf = lds + ((u + sb) & 1) * STAGE;
            const float4* sa = sbuf + (wm * 128) * 8;
            const float4* sw = sbuf + SA + (wn * 64) * 8;
            const int g1 = u + 1, g2 = u + 2;               // K-tiles the DMAs of this K-tile belong to (>= nkt: the next unit's)
            const bool i1 = g1 < nkt || stream, i2 = g2 < nkt || stream;
            const int k1 = g1 < nkt ? g1 : g1 - nkt, k2 = g2 < nkt ? g2 : g2 - nkt;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                // ---------------- L-segment
                if (p == 0) {
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int n = 0; n < 2; ++n)
#pragma unroll
                            for (int ks = 0; ks < 2; ++ks) {
                                const float4 v = sw[((j * 2 + n) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                                if (j == 0) bf0[n][ks] = *reinterpret_cast<const v8*>(&v);
                                else        bf1[n][ks] = *reinterpret_cast<const v8*>(&v);
                            }
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)      // A fragments of the 64-row half i = p
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const float4 v = sa[((p * 4 + m) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                        af[m][ks] = *reinterpret_cast<const v8*>(&v);
                    }
                __builtin_amdgcn_sched_barrier(0);
                if (p == 0 && i1) { issue_half(0, k1, (g1 + sb) & 1); issue_half(1, k1, (g1 + sb) & 1); }
                if (p == 1 && stream && u == nkt - 2) set_tile(nx_tile, 0);   // this unit's last DMA is out: the next unit's addresses
                if (p == 1 && i2) { issue_half(2, k2, (g2 + sb) & 1); issue_half(3, k2, (g2 + sb) & 1); }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this phase's reads are in registers before anyone may refill
                if (p == 1 && wm == 1) {     // the late group confirms K-tile u+1 at the end of its L(2u+1) ...
                    if (i2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                // ---------------- C-segment: quadrants (i = p, j = 0) and (i = p, j = 1)
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
                            acc[n][p * 4 + m] = X16<T>::mfma(bf0[n][ks], af[m][ks], acc[n][p * 4 + m]);
                            acc[2 + n][p * 4 + m] = X16<T>::mfma(bf1[n][ks], af[m][ks], acc[2 + n][p * 4 + m]);
                        }
                __builtin_amdgcn_s_setprio(0);
                if (p == 1 && wm == 0) {     // ... the early group at the end of its C(2u+1): the same interval
                    if (i2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
            }
        }
        } else if (!halfu) {
        for (int u = 0; u < nkt; ++u) {
            const float4* sbuf = lds + ((u + sb) & 1) * STAGE;
            const float4* sa = sbuf + (wm * 128) * 8;
            const float4* sw = sbuf + SA + (wn * 64) * 8;
            const int g1 = u + 1, g2 = u + 2;               // K-tiles the DMAs of this K-tile belong to (>= nkt: the next unit's)
            const bool i1 = g1 < nkt || stream, i2 = g2 < nkt || stream;
            const int k1 = g1 < nkt ? g1 : g1 - nkt, k2 = g2 < nkt ? g2 : g2 - nkt;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                // ---------------- L-segment
                if ((p == 0 || p == 1) && !PH_ABLATE(1)) {      // W fragments of the 32-column half j = p
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const float4 v = sw[((p * 2 + n) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                            if (p == 0) bf0[n][ks] = *reinterpret_cast<const v8*>(&v);
                            else        bf1[n][ks] = *reinterpret_cast<const v8*>(&v);
                        }
                }
                if ((p == 0 || p == 2) && !PH_ABLATE(1)) {      // A fragments of the 64-row half i = p / 2
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const float4 v = sa[(((p >> 1) * 4 + m) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                            af[m][ks] = *reinterpret_cast<const v8*>(&v);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (!PH_ABLATE(0)) {
                if (p == 0 && i1) issue_half(3, k1, (g1 + sb) & 1);
                if (p == 1 && stream && u == nkt - 2) set_tile(nx_tile, 0);   // this unit's last DMA is out: the next unit's addresses
                if (p == 2 && i2) issue_half(2, k2, (g2 + sb) & 1);
                if (p == 3 && i2) { issue_half(0, k2, (g2 + sb) & 1); issue_half(1, k2, (g2 + sb) & 1); }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this phase's reads are in registers before anyone may refill
                if (p == 3 && wm == 1) {     // the late group confirms K-tile u+1 at the end of its L(4u+3) ...
                    if (i2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                // ---------------- C-segment: quadrant (i, j) = (0,0) (0,1) (1,1) (1,0)
                __builtin_amdgcn_s_setprio(1);
                if (!PH_ABLATE(2))
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
                            const int i = p >> 1, j = (p == 1 || p == 2) ? 1 : 0;
                            const v8 wv = j ? bf1[n][ks] : bf0[n][ks];
                            acc[j * 2 + n][i * 4 + m] = X16<T>::mfma(wv, af[m][ks], acc[j * 2 + n][i * 4 + m]);
                        }
                __builtin_amdgcn_s_setprio(0);
                if (p == 3 && wm == 0) {     // ... the early group at the end of its C(4u+3): the same interval
                    if (i2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
            }
        }
        } else {
        int st3 = 0, st3n = 2;                                // ring slots of K-tile u and of K-tile u + 2
        for (int u = 0; u < nkt; ++u) {
            const float4* sb = lds + st3 * HSTAGE;
            const float4* sa = sb + (wm * 64) * 8;
            const float4* sw = sb + HSA + (wn * 64) * 8;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                // ---------------- L-segment
#pragma unroll
                for (int n = 0; n < 2; ++n)      // W fragments of the 32-column half j = p
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const float4 v = sw[((p * 2 + n) * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                        if (p == 0) bf0[n][ks] = *reinterpret_cast<const v8*>(&v);
                        else        bf1[n][ks] = *reinterpret_cast<const v8*>(&v);
                    }
                if (p == 0) {                    // A fragments: the wave's 64 rows
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const float4 v = sa[(m * 16 + c) * 8 + ((ks * 4 + g) ^ (c & 7))];
                            af[m][ks] = *reinterpret_cast<const v8*>(&v);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (p == 0 && u + 2 < nkt) issue_h(0, u + 2, st3n);                                 // A first: the operand that misses L2
                if (p == 1 && u + 2 < nkt) { issue_h(2, u + 2, st3n); issue_h(3, u + 2, st3n); }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (p == 1 && wm == 1) {     // the late group confirms K-tile u+1 at the end of its L(2u+1) ...
                    if (u + 2 < nkt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                // ---------------- C-segment: quadrant (0, j = p)
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
                            const v8 wv = p ? bf1[n][ks] : bf0[n][ks];
                            acc[p * 2 + n][m] = X16<T>::mfma(wv, af[m][ks], acc[p * 2 + n][m]);
                        }
                __builtin_amdgcn_s_setprio(0);
                if (p == 1 && wm == 0) {     // ... the early group at the end of its C(2u+1): the same interval
                    if (u + 2 < nkt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
            }
            st3 = st3 == 2 ? 0 : st3 + 1;
            st3n = st3n == 2 ? 0 : st3n + 1;
        }
        }
        if (wm == 0 && (PH != 1 || halfu)) __builtin_amdgcn_s_barrier();   // the early group waits out the late group's last C-segment
        PH_STAMP(sbase + 2);                                // K loop done

        // Both operand stages are free now (every read of the last K-tiles completed before the barriers above).  Epilogues without a
        // residual put the NEXT unit's first DMAs in flight right here, so their latency runs under the whole epilogue.  The residual
        // epilogues (RESV) first request ALL residual rows of the unit and issue those DMAs one LDS pass later, behind an explicit
        // wait: hipcc counts only the loads it can see, so with hidden DMAs in flight every wait it inserts for a residual row is a
        // wait for (most of) the DMAs too, and vmcnt retires in order anyway -- round 2 prefetched the residual one pass ahead and
        // in-kernel stamps (tools/gemm_bf16_stamps.py) showed every pass of an epilogue-5 tile sitting through a 2-3 us round trip
        // (16.5 us outside the K loop against 6.5 for epilogue 0).  The residual rows of passes 0 and 1 are requested up front (older
        // than the DMAs); those of pass k + 2 at the end of pass k, into the registers it has freed -- younger than the DMAs, which
        // have had two passes to land by the time these are waited for.  (All four passes up front: 96 more live registers, 40 spilled.)
        float4 bv[4];                                          // !RESV: this unit's bias for the lane's 4 x 4 columns, before the DMAs
        if (!RESV) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = cn0 + wn * 64 + n * 16 + 4 * g;
                bv[n] = (bias && col < N) ? ld4(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        ++ui;
        have = nx_have;
        cur_tile = nx_tile; cur_mode = nx_mode;
        if (have && !stream) set_tile(nx_tile, nx_mode);   // (stream: done inside the K loop, and the next unit's K-tile 0 has landed)
        if (!RESV && have && !stream) issue_prologue(KT, nx_mode);
        sb = stream ? (sb + nkt) & 1 : 0;
        streamed_in = stream;

        const int kpass = halfu ? 2 : 4;                       // epilogue passes of 2 m-tiles per wave row (a half unit has 4 m-tiles)
        PH_STAMP(sbase + 3);                                // next unit's prologue issued (RESV: only its addresses are ready)
        // Epilogue through the 32 KB C stage in 4 passes of 64 rows (m-tiles 2k, 2k+1 of both wave rows): bias / GELU in registers,
        // bf16 rows staged with the 16-byte chunk XOR-swizzled by the row (the 16 rows a ds_write touches would otherwise share
        // their banks: the row pitch is 512 B), streamed out as whole rows, 16 bytes per lane; the residual (and, with it, the bias)
        // is added on the way out.  Raw barriers + lgkmcnt only: a __syncthreads() would wait for the DMAs in flight.
        unsigned char* sC = reinterpret_cast<unsigned char*>(lds + CST);
        // LayerNorm folded into this GEMM (LNF): this lane's rows' (mean, rstd) and its columns' c1 = sum_k W'[n, k]
        float mu[8], rs[8];
        float4 c1v[4];
        if (LNF) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                int row = cm0 + wm * wrows + m * 16 + c;
                row = row < M ? row : M - 1;
                const float2 st = *reinterpret_cast<const float2*>(ln.rowstat + (int64_t)row * 2);
                mu[m] = st.x; rs[m] = st.y;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = cn0 + wn * 64 + n * 16 + 4 * g;
                c1v[n] = col < N ? ld4(ln.c1 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        // RES_LN: the residual is LayerNorm(res row) -- the raw row comes with its (mean, rstd); gamma / beta of this thread's 8
        // columns are loaded once per unit (a thread keeps its 16-byte chunk index through all passes), the bias joins beta.
        // (An already-normalised residual comes with identity tables -- mean 0, rstd 1, gamma 1, beta 0 -- not with a null pointer.
        // N % 256 == 0 for the LayerNorm epilogues, so the 8 columns are always in range; the plain residual epilogue clamps.)
        v8 rr[2][4];                                          // ring of two passes
        f32x2 ss[2][4];
        auto load_res = [&](int k, v8 (&rd)[4], f32x2 (&sd)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int id = tid + i * 512, prow = id >> 5, ch = id & 31;
                const int lrow = (prow >> 5) * wrows + (2 * k + ((prow >> 4) & 1)) * 16 + (prow & 15);
                int row = cm0 + lrow, col = cn0 + ch * 8;
                row = row < M ? row : M - 1; col = col < N ? col : 0;         // clamped: loaded, not used
                rd[i] = *reinterpret_cast<const v8*>(res + (int64_t)row * ldc + col);
                if (EPI == BEPI_RES_LN) sd[i] = *reinterpret_cast<const f32x2*>(ln.rowstat + (int64_t)row * 2);
            }
        };
        const int my_col = cn0 + (tid & 31) * 8;
        f32x4 gam0, gam1, bet0, bet1;
        if (RESV) {
            auto ldv4 = [](const float* p) { return *reinterpret_cast<const f32x4*>(p); };
            const int bc = my_col < N ? my_col : 0;
            bet0 = bias ? ldv4(bias + bc) : (f32x4){0.f, 0.f, 0.f, 0.f};
            bet1 = bias ? ldv4(bias + bc + 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
            if (EPI == BEPI_RES_LN) {
                gam0 = ldv4(ln.ln_g + my_col); gam1 = ldv4(ln.ln_g + my_col + 4);
                bet0 += ldv4(ln.ln_b + my_col); bet1 += ldv4(ln.ln_b + my_col + 4);
            }
            load_res(0, rr[0], ss[0]);
            load_res(1, rr[1], ss[1]);                         // (kpass >= 2 always)
        }
        if constexpr (EPI != BEPI_BIAS_F32) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= kpass) break;                            // workgroup-uniform
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                const int m = 2 * k + mm;
                const int prow = (wm * 2 + mm) * 16 + c;      // row inside the pass
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int lcol = wn * 64 + n * 16 + 4 * g;
                    float4 v = make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]);
                    if (LNF)   // rstd (A W'^T - mean c1) + c2, c2 in the bias slot
                        v = make_float4(rs[m] * fmaf(-mu[m], c1v[n].x, v.x), rs[m] * fmaf(-mu[m], c1v[n].y, v.y),
                                        rs[m] * fmaf(-mu[m], c1v[n].z, v.z), rs[m] * fmaf(-mu[m], c1v[n].w, v.w));
                    if (!RESV) v = add4(v, bv[n]);
                    if (EPI == BEPI_BIAS_GELU || EPI == BEPI_LNFOLD_GELU) {
                        const f32x2 g0 = gelu_fast2((f32x2){v.x, v.y}), g1 = gelu_fast2((f32x2){v.z, v.w});
                        v = make_float4(g0[0], g0[1], g1[0], g1[1]);
                    }
                    v4 o = {(T)v.x, (T)v.y, (T)v.z, (T)v.w};
                    const int ch = (lcol >> 3) ^ (prow & 31);
                    *reinterpret_cast<v4*>(sC + prow * 512 + ch * 16 + (lcol & 7) * 2) = o;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            PH_STAMP(sbase + 4 + 2 * k);                        // pass k staged
            if (RESV && k == 0) {
                // every residual chunk of the unit has landed (and the compiler is told so: the empty statements "write" the registers,
                // so no wait of its own can follow once the hidden DMAs are in flight); only now the next unit's first DMAs
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        asm volatile("" : "+v"(rr[kk][i]));
                        if (EPI == BEPI_RES_LN) asm volatile("" : "+v"(ss[kk][i]));
                    }
                asm volatile("" : "+v"(bet0), "+v"(bet1));
                if (EPI == BEPI_RES_LN) asm volatile("" : "+v"(gam0), "+v"(gam1));
                if (have && !stream) issue_prologue(KT, nx_mode);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                      // 64 rows x 32 chunks = 2048 chunks / 512 threads
                const int id = tid + i * 512, prow = id >> 5, ch = id & 31;
                const int lrow = (prow >> 5) * wrows + (2 * k + ((prow >> 4) & 1)) * 16 + (prow & 15);
                const int row = cm0 + lrow, col = cn0 + ch * 8;
                const bool inb = row < M && col < N;
                // The read-out side works on PAIRS with packed fp32 arithmetic (v_pk_fma_f32 / v_pk_add_f32: fine in an epilogue, an
                // anti-lever beside MFMAs): epilogue 5 was ~2200 VALU instructions per wave and tile more than epilogue 0, ~9 us of the
                // 17 us an out-proj tile spent outside its K loop.  A bf16 pair sits in one dword: lo << 16 and hi & 0xffff0000 are
                // the two fp32 values.
                u32x4 vw = *reinterpret_cast<const u32x4*>(sC + prow * 512 + ((ch ^ (prow & 31)) * 16));
                if (RESV) {
                    const u32x4 rw = __builtin_bit_cast(u32x4, rr[k & 1][i]);
                    // LayerNorm of the residual row: (r - mean) rstd gamma + beta = (r a + b) gamma + beta with a = rstd, b = -mean rstd
                    // (beta carries the GEMM's bias too)
                    const float ra = ss[k & 1][i][1], rb = -ss[k & 1][i][0] * ss[k & 1][i][1];
                    const f32x2 gam2[4] = {{gam0[0], gam0[1]}, {gam0[2], gam0[3]}, {gam1[0], gam1[1]}, {gam1[2], gam1[3]}};
                    const f32x2 bet2[4] = {{bet0[0], bet0[1]}, {bet0[2], bet0[3]}, {bet1[0], bet1[1]}, {bet1[2], bet1[3]}};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x2 x = X16<T>::unpack(vw[q]);
                        f32x2 r = X16<T>::unpack(rw[q]);
                        if (EPI == BEPI_RES_LN) {
                            r = __builtin_elementwise_fma(r, (f32x2){ra, ra}, (f32x2){rb, rb});
                            r = __builtin_elementwise_fma(r, gam2[q], bet2[q]);
                        } else {
                            r = r + bet2[q];                           // the bias
                        }
                        x = x + r;
                        if constexpr (!X16<T>::is_bf16) {   // fp16 residual stream of the decoder's big prefill: saturate instead of inf -> NaN
                            x[0] = __builtin_amdgcn_fmed3f(x[0], -65504.f, 65504.f);   // (bf16 has fp32's range)
                            x[1] = __builtin_amdgcn_fmed3f(x[1], -65504.f, 65504.f);
                        }
                        const v2 o = {(T)x[0], (T)x[1]};
                        vw[q] = __builtin_bit_cast(unsigned, o);
                    }
                }
                if (inb) *reinterpret_cast<u32x4*>(C + (int64_t)row * ldc + col) = vw;
                if (EPI == BEPI_RES_LN && ln.stats_out) {
                    // (sum, M2 = sum of squared deviations from the TILE's mean) of the row's 256 bf16 outputs in this tile (N % 256 == 0
                    // for this epilogue: every tile has 256 valid columns); the row's 32 chunks sit in 32 consecutive lanes.  Deviations
                    // from the tile mean, not raw squares: E[x^2] - mean^2 in fp32 loses the variance of a row whose mean is large
                    // against its spread (outlier hidden dimensions of trained checkpoints); ln_rowstat merges the tiles exactly (Chan).
                    // (rows beyond M compute garbage that is never stored)
                    f32x2 s1p = {0.f, 0.f}, s2p = {0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < 4; ++q) s1p += X16<T>::unpack(vw[q]);
                    const float s1 = half_wave_sum(s1p[0] + s1p[1]);
                    const float tmean = s1 * (1.0f / 256.0f);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x2 d = X16<T>::unpack(vw[q]) - (f32x2){tmean, tmean};
                        s2p = __builtin_elementwise_fma(d, d, s2p);
                    }
                    const float s2 = half_wave_sum(s2p[0] + s2p[1]);
                    if (ch == 0 && row < M)
                        *reinterpret_cast<float2*>(ln.stats_out + ((int64_t)row * tiles_n + (cn0 >> 8)) * 2) = make_float2(s1, s2);
                }
            }
            if (RESV && k + 2 < kpass) load_res(k + 2, rr[k & 1], ss[k & 1]);   // the slot this pass has just consumed
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                     // the C stage is rewritten by the next pass
            PH_STAMP(sbase + 5 + 2 * k);                        // pass k read out, stores issued
        }
        } else {
            // fp32 rows: 8 passes (4 for a half unit) of 32 rows -- m-tile k of both wave rows -- through the same 32 KB C stage:
            // 32 rows x 1 KB, the 16-byte chunk XOR-swizzled by the row (the 16 rows a ds_write_b128 touches would share their
            // banks: the row pitch is a multiple of the 256-byte bank row), streamed out as whole rows, 16 bytes per lane.
            float* Cf = reinterpret_cast<float*>(C);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < 2 * kpass) {                              // workgroup-uniform (no `break`: hipcc then leaves the loop rolled and acc[n][k] goes to scratch)
                const int prow = wm * 16 + c;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int lcol = wn * 64 + n * 16 + 4 * g;
                    const float4 v = add4(make_float4(acc[n][k][0], acc[n][k][1], acc[n][k][2], acc[n][k][3]), bv[n]);
                    *reinterpret_cast<float4*>(sC + prow * 1024 + (((lcol >> 2) ^ (prow & 15)) * 16)) = v;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
#pragma unroll
                for (int i = 0; i < 4; ++i) {                      // 32 rows x 64 chunks = 2048 chunks / 512 threads
                    const int id = tid + i * 512, pr = id >> 6, ch = id & 63;
                    const int row = cm0 + (pr >> 4) * wrows + k * 16 + (pr & 15), col = cn0 + ch * 4;
                    const float4 v = *reinterpret_cast<const float4*>(sC + pr * 1024 + ((ch ^ (pr & 15)) * 16));
                    // 2.2 GB of logits at the decoder's [64, 1024] prefill that no kernel of the forward reads back: non-temporal stores
                    if (row < M && col < N) __builtin_nontemporal_store(*reinterpret_cast<const f32x4*>(&v), reinterpret_cast<f32x4*>(Cf + (int64_t)row * ldc + col));
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                     // the C stage is rewritten by the next pass
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// TWO WORKGROUPS PER CU ("duo"): 256 x 128 of C per workgroup of 4 waves (2 x 2, the same 128 x 64 per wave and the same fragment
// layout as the 256 x 256 kernel), 80 KB of LDS each, so that a CU holds two of them and they run INDEPENDENTLY: while one is in
// its epilogue (VALU, LDS, global stores; matrix pipe idle), waiting at a barrier or for its fragments, the other one's waves have the
// matrix pipe of every SIMD to themselves.  The 8-wave kernel above is one workgroup whose waves all reach the epilogue together:
// stamps put 24-42 % of a tile's time outside the K loop at K = 768 (VERDICT r2 #2 asks for exactly this overlap).  Price: the tile
// has 1.5 x the operand bytes per FLOP.
//   LDS  : K-tiles of 64 (whole 128-byte lines per row: a first version with K-steps of 32 and a three-stage ring made 64-byte requests,
//          3 x the L2 requests of the 256 x 256 kernel per FLOP, and ran at 0.77 of its rate -- profiles/r3_gemm_duo_bk32_*).  80 KB hold
//          TWO A stages (256 rows x 128 B = 32 KB each) and ONE W buffer (128 rows, 16 KB): W is the operand that sits in L2, its K-tile
//          is read into registers (8 fragments, both k-steps) at the top of a K-tile and refilled behind a second barrier.
//   loop : K-tile u: vmcnt(0) [A(u), W(u): nothing younger], barrier B1 (publishes them; A stage (u+1) & 1 is free: every wave has left
//          K-tile u-1); read the 8 W fragments and the 8 A fragments of k-step 0; lgkmcnt(0), barrier B2 (the W buffer is free);
//          then 64 MFMAs, m-tile by m-tile, with the A fragments of k-step 1 refilled in place behind their last use, and among them
//          this wave's 8 pieces of A(u+1) and 4 of W(u+1).  The exposed reads at the top are what the OTHER workgroup covers.
//   tile : the whole 256 x 128 bf16 tile (64 KB) is staged through the two A stages after the K loop, one barrier, whole-row stores.
// MEASURED (round 3, in-process A/B against the 256 x 256 kernel, outputs bitwise equal; profiles/r3_gemm_duo_*): 0.92 of its rate on QKV
// (K = 768), 0.91 on FC1 with GELU -- the GELU costs this kernel what it costs the other one, nothing hides it --, 0.99 on the out-proj shape,
// 0.93 at K = 3072; 1.25 x at K = 192 and 1.05 x at 8192^3.  Delaying one workgroup of every CU by 4-16 us changes nothing.  NOT the engine's
// choice: switch bf16_gemm_tile = 5, plain epilogues (bias, bias + GELU) only.
template <int EPI, typename T>
__global__ __launch_bounds__(256, 2) void gemm16_duo_kernel(const T* __restrict__ A, int lda, const T* __restrict__ W, int ldw,
                                                           const float* __restrict__ bias, const T* __restrict__ res,
                                                           T* __restrict__ C, int ldc, int M, int N, int K, int tiles_n, int n_tiles) {
    typedef typename X16<T>::v8 v8;
    typedef typename X16<T>::v4 v4;
    constexpr int BM = 256, BN = 128;
    constexpr int SA = BM * 8, WOFF = 2 * SA;               // in 16-byte chunks: two A stages, then the W buffer
    extern __shared__ __attribute__((aligned(16))) float4 lds[];   // 80 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int KT = K >> 6;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float4*)lds;
    // the XCD's contiguous run of tiles, walked with stride gridDim.x / 8 (speed only)
    const int wg_x = gridDim.x >> 3, slot = (int)blockIdx.x >> 3;
    const int run_len = (n_tiles + 7) >> 3, run0 = ((int)blockIdx.x & 7) * run_len;
    const int per_x = run0 + run_len < n_tiles ? run_len : n_tiles - run0;
    // fragment reads: row c of a 16-row tile, chunk (ks * 4 + g) ^ (c & 7); DMA pieces of 8 rows: lane -> row lane / 8, chunk (lane % 8) ^ row
    const int fr0 = c * 8 + (g ^ (c & 7)), fr1 = c * 8 + ((4 + g) ^ (c & 7));
    const int lr = lane >> 3, lch = (lane & 7) ^ lr;
    for (int it = slot; it < per_x; it += wg_x) {
        int t = run0 + it;
        asm volatile("" : "+s"(t));                           // (opaque: keeps the per-tile address arithmetic inside the tile loop)
        const int m0 = (t / tiles_n) * BM, n0 = (t % tiles_n) * BN;
        unsigned voa[8], vow[4];                              // this wave's pieces: A rows (8 w + i) * 8 .., W rows (4 w + i) * 8 ..
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int r = (wave * 8 + i) * 8 + lr;
            r = m0 + r < M ? r : M - 1 - m0;
            voa[i] = (unsigned)(r * lda + lch * 8) * 2u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r = (wave * 4 + i) * 8 + lr;
            r = n0 + r < N ? r : N - 1 - n0;
            vow[i] = (unsigned)(r * ldw + lch * 8) * 2u;
        }
        const char* abase = reinterpret_cast<const char*>(A + (int64_t)m0 * lda);
        const char* wbase = reinterpret_cast<const char*>(W + (int64_t)n0 * ldw);
        auto issue_a = [&](int i, int kt, int st) {
            glds16_hidden_s(abase + kt * 128, voa[i], lds_base + (unsigned)(st * SA + (wave * 8 + i) * 64) * 16u);
        };
        auto issue_w = [&](int i, int kt) {
            glds16_hidden_s(wbase + kt * 128, vow[i], lds_base + (unsigned)(WOFF + (wave * 4 + i) * 64) * 16u);
        };
#pragma unroll
        for (int i = 0; i < 4; ++i) issue_w(i, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) issue_a(i, 0, 0);
        f32x4 acc[4][8];
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto rd = [&](const float4* p_) -> v8 { const float4 v = *p_; return *reinterpret_cast<const v8*>(&v); };
        for (int u = 0; u < KT; ++u) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of A(u), W(u) (and, at u = 0, the previous tile's stores)
            __builtin_amdgcn_s_barrier();                        // B1
            const float4* sa = lds + (u & 1) * SA + (wm * 128) * 8;
            const float4* sw = lds + WOFF + (wn * 64) * 8;
            v8 fw[2][4], fa[8];
#pragma unroll
            for (int n = 0; n < 4; ++n) { fw[0][n] = rd(sw + n * 128 + fr0); fw[1][n] = rd(sw + n * 128 + fr1); }
#pragma unroll
            for (int m = 0; m < 8; ++m) fa[m] = rd(sa + m * 128 + fr0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();                        // B2: every wave holds W(u) in registers
            const bool nx = u + 1 < KT;
            const int st1 = (u + 1) & 1;
#pragma unroll
            for (int m = 0; m < 8; ++m) {                        // k-step 0
                if (nx) issue_a(m, u + 1, st1);
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n][m] = X16<T>::mfma(fw[0][n], fa[m], acc[n][m]);
                fa[m] = rd(sa + m * 128 + fr1);                   // k-step 1's fragment, in place behind the last use
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {                        // k-step 1
                if (nx && m < 4) issue_w(m, u + 1);
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n][m] = X16<T>::mfma(fw[1][n], fa[m], acc[n][m]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // epilogue: the tile as bf16 through the two A stages (row pitch 256 B, 16-byte chunk XOR-swizzled by the row), whole-row stores
        __builtin_amdgcn_s_barrier();                         // every wave has read its last fragments
        unsigned char* sC = reinterpret_cast<unsigned char*>(lds);
        int tid_o = tid, c_o = c, g_o = g;                    // opaque per-tile copies: hipcc otherwise computes every epilogue address
        asm volatile("" : "+v"(tid_o), "+v"(c_o), "+v"(g_o));  // (thread-index-only arithmetic) before the K loop and keeps it live through it
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int lcol = wn * 64 + n * 16 + 4 * g_o;
            const int col = n0 + lcol;
            const float4 bv = (bias && col < N) ? ld4(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int row = wm * 128 + m * 16 + c_o;
                float4 v = add4(make_float4(acc[n][m][0], acc[n][m][1], acc[n][m][2], acc[n][m][3]), bv);
                if (EPI == BEPI_BIAS_GELU) {
                    const f32x2 g0 = gelu_fast2((f32x2){v.x, v.y}), g1 = gelu_fast2((f32x2){v.z, v.w});
                    v = make_float4(g0[0], g0[1], g1[0], g1[1]);
                }
                v4 o = {(T)v.x, (T)v.y, (T)v.z, (T)v.w};
                *reinterpret_cast<v4*>(sC + row * 256 + (((lcol >> 3) ^ (row & 15)) * 16) + (lcol & 7) * 2) = o;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < 16; ++i) {                        // 256 rows x 16 chunks / 256 threads
            const int id = tid_o + i * 256, row = id >> 4, ch = id & 15;
            const u32x4 vw = *reinterpret_cast<const u32x4*>(sC + row * 256 + ((ch ^ (row & 15)) * 16));
            const int grow = m0 + row, gcol = n0 + ch * 8;
            if (grow < M && gcol < N) *reinterpret_cast<u32x4*>(C + (int64_t)grow * ldc + gcol) = vw;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // the stages are free for the next tile's first pieces
    }
}

// ------------------------------------------------------------------------------------------
// the instantiation a plan names ({nullptr, nullptr}: none)
template <int EPI, typename T>
static KernelRef gemm16_ph(int phases) {
    if (phases == 1) return kernel_ref<&gemm_bf16_ph_kernel<EPI, T, 1>>();
    if (phases == 2) return kernel_ref<&gemm_bf16_ph_kernel<EPI, T, 2>>();
    return kernel_ref<&gemm_bf16_ph_kernel<EPI, T, 4>>();
}
template <int EPI>
static KernelRef gemm16_epi(const Gemm16Plan& p) {
    if constexpr (EPI == BEPI_BIAS_F32) return p.f16 ? gemm16_ph<EPI, _Float16>(p.phases) : KernelRef{};
    else if constexpr (EPI >= BEPI_LNFOLD) return p.f16 ? gemm16_ph<EPI, _Float16>(p.phases) : gemm16_ph<EPI, bf16_t>(p.phases);
    else {
        if (p.f16) return KernelRef{};
        switch (p.family) {
            case G16_SMALL: return kernel_ref<&gemm_bf16_nt_kernel<EPI>>();
            case G16_PERSISTENT: return gemm16_ph<EPI, bf16_t>(p.phases);
            case G16_DUO: return kernel_ref<&gemm16_duo_kernel<EPI, bf16_t>>();   // (never planned with BEPI_BIAS_RES)
        }
        if (p.nt == 4) return kernel_ref<&gemm_bf16_glds_kernel<EPI, 4, 2>>();
        return p.wmw == 1 ? kernel_ref<&gemm_bf16_glds_kernel<EPI, 2, 1>>() : kernel_ref<&gemm_bf16_glds_kernel<EPI, 2, 2>>();
    }
}
static KernelRef gemm16_kernel(const Gemm16Plan& p) {
    switch (p.epi) {
        case BEPI_BIAS: return gemm16_epi<BEPI_BIAS>(p);
        case BEPI_BIAS_GELU: return gemm16_epi<BEPI_BIAS_GELU>(p);
        case BEPI_BIAS_RES: return gemm16_epi<BEPI_BIAS_RES>(p);
        case BEPI_LNFOLD: return gemm16_epi<BEPI_LNFOLD>(p);
        case BEPI_LNFOLD_GELU: return gemm16_epi<BEPI_LNFOLD_GELU>(p);
        case BEPI_RES_LN: return gemm16_epi<BEPI_RES_LN>(p);
        case BEPI_BIAS_F32: return gemm16_epi<BEPI_BIAS_F32>(p);
    }
    return KernelRef{};
}

static Gemm16Switches gemm16_switches() {
    return Gemm16Switches{tune(TUNE_BF16_GEMM_TILE), tune(TUNE_BF16_GEMM_SMALL), tune(TUNE_BF16_GEMM_TAIL), tune(TUNE_BF16_GEMM_PHASES),
                          tune(TUNE_BF16_GEMM_REVERSE)};
}

bool gemm_bf16_is_persistent(int M, int N, int K) {
    DeviceInfo di;
    if (device_info(&di) != MGEA_OK) return false;
    const Gemm16Call c{M, N, K, 8, 8, 8, BEPI_BIAS};
    Gemm16Plan p;
    return plan_gemm16(c, gemm16_switches(), di.n_cu, &p, nullptr) == 0 && p.family == G16_PERSISTENT;
}

int launch_gemm_bf16(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res, void* C,
                     int ldc, int M, int N, int K, int epi, hipStream_t st, GemmBf16Info* info, const BfEpiLn* lnp, int f16, int reverse) {
    BfEpiLn ln = lnp ? *lnp : BfEpiLn{nullptr, nullptr, nullptr, nullptr, nullptr};
    const Gemm16Call c{M, N, K, lda, ldw, ldc, epi, f16 != 0, bias != nullptr, res != nullptr, ln.rowstat != nullptr, ln.c1 != nullptr,
                       ln.ln_g != nullptr, ln.ln_b != nullptr, ln.stats_out != nullptr, reverse != 0};
    DeviceInfo di;
    MGEA_TRY(device_info(&di));
    Gemm16Plan p;
    const char* why = "";
    MGEA_REQUIRE(plan_gemm16(c, gemm16_switches(), di.n_cu, &p, &why) == 0, MGEA_EINVAL, "16-bit gemm M=%d N=%d K=%d ldc=%d epilogue %d%s: %s",
                 M, N, K, ldc, epi, f16 ? " (fp16)" : "", why);
    if (info) { info->kernel = p.family; info->half_tiles = p.half_tiles; info->tail_mode = p.tail_mode; }
    const KernelRef k = gemm16_kernel(p);
    MGEA_REQUIRE(k.fn, MGEA_EINVAL, "16-bit gemm: no kernel for plan family %d, epilogue %d", p.family, epi);
    if (p.shmem) MGEA_TRY(set_max_dynamic_lds(k.fn, p.shmem, di.dev, k.lds_raised));
    // one argument list for the four families: each kernel takes a prefix of it (small, ring: up to tiles_n; duo: n_tiles; persistent: all)
    void* args[] = {&A, &lda, &W, &ldw, &bias, &res, &C, &ldc, &M, &N, &K, &p.tiles_n, &p.n_tiles, &p.tail_mode, &ln};
    MGEA_CHECK_HIP(hipLaunchKernel(k.fn, dim3(p.grid), dim3(p.block), args, p.shmem, st));
    return MGEA_OK;
}
}  // namespace mgea
