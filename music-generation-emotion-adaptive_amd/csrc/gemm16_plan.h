// The launch plan of the 16-bit GEMMs (gemm16.hip): plan_gemm16 makes every choice of a launch_gemm_bf16 call -- kernel family,
// template parameters, geometry, the tail word of the persistent kernel -- and holds every shape / operand refusal, once for bf16
// and fp16; launch_gemm_bf16 launches exactly that plan.  Plain C++17, no HIP include: tests/native/gemm16_plan_test.cpp compiles
// it for the host alone.
#pragma once
#include <stdint.h>

namespace mgea {

// epilogues of launch_gemm_bf16: out = epi(A W^T + bias)
enum { BEPI_BIAS = 0, BEPI_BIAS_GELU = 1, BEPI_BIAS_RES = 2,
       // LayerNorm folded around the GEMMs (persistent 256 x 256 kernel only; see BfEpiLn in common.h):
       BEPI_LNFOLD = 3,        // out = rstd_row (A W'^T - mean_row c1) + c2         (A = raw rows, W' = W diag(gamma), c2 in the bias slot)
       BEPI_LNFOLD_GELU = 4,   // ... then GELU
       BEPI_RES_LN = 5,        // out = A W^T + bias + LN(res rows) (LayerNorm of the residual applied on the way in), + row statistics of out
       BEPI_BIAS_F32 = 6 };    // out = A W^T + bias written as fp32 [M, ldc floats] (the decoder's LM head: N = vocab need only be a multiple of 4)

// kernel families, the numbers GemmBf16Info.kernel reports: gemm_bf16_nt_kernel (register-staged 128 x 128), gemm_bf16_glds_kernel
// (the LDS-DMA ring kernels), gemm_bf16_ph_kernel (persistent, phase-interleaved 256 x 256), gemm16_duo_kernel (two workgroups per CU)
enum { G16_SMALL = 0, G16_RING = 1, G16_PERSISTENT = 2, G16_DUO = 3 };

// what a caller asks for; the optional operands (bias, residual, the BfEpiLn pointers) as "present"
struct Gemm16Call {
    int M, N, K, lda, ldw, ldc;
    int epi;                 // BEPI_*
    bool f16;                // _Float16 operands (else bf16)
    bool bias, res, rowstat, c1, ln_g, ln_b, stats_out;
    bool reverse;            // A is the previous kernel's large output: walk the tiles from the end of every XCD's run (persistent kernel)
};
// the TUNE_BF16_GEMM_* switches (common.h)
struct Gemm16Switches { int tile, small, tail, phases, reverse; };
// what will run
struct Gemm16Plan {
    int family;              // G16_*
    int epi; bool f16;       // with the three below: the instantiation (gemm16_kernel)
    int nt, wmw;             // ring: gemm_bf16_glds_kernel<epi, nt, wmw>
    int phases;              // persistent: gemm_bf16_ph_kernel<epi, T, phases>
    int tail_mode;           // persistent: bits 0-1 the tail schedule (switch bf16_gemm_tail), bit 2 the reversed walk
    int half_tiles;          // persistent: 1 when the tiles left after the full rounds run as two 128-row halves
    int tiles_n, n_tiles;    // column tiles and tiles of the family's tile shape (kernel arguments)
    int grid, block, shmem;  // shmem: dynamic LDS bytes (0: none, no limit to raise)
};

// The persistent kernel's HALF-TILE TAIL, as the kernel computes it for XCD run 0 (the longest): the tiles the run leaves after the
// full rounds of its grid / 8 workgroups are cut into two 128-row halves when the tail schedule allows it and they number at most half
// the workgroups.  (The kernel keeps its own three lines: written as a call of one shared function, hipcc turned one of its unsigned
// compares into a signed one.  tests/native/gemm16_plan_test.cpp holds this function to the kernel's arithmetic.)
inline int gemm16_half_tiles(int n_tiles, int grid, int tail_mode) {
    const int wg_x = grid / 8, per_x = (n_tiles + 7) / 8 < n_tiles ? (n_tiles + 7) / 8 : n_tiles;
    const int rem = per_x - per_x / wg_x * wg_x;
    return ((tail_mode & 3) != 0 && rem > 0 && 2 * rem <= wg_x) ? 1 : 0;
}

// 0 and *p filled, or 1 and *why (if given) naming the refusal.  n_cu: compute units of the device.
inline int plan_gemm16(const Gemm16Call& c, const Gemm16Switches& sw, int n_cu, Gemm16Plan* p, const char** why) {
    const auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    const auto up8 = [](int x) { return (x + 7) / 8 * 8; };
    const auto refuse = [&](const char* w) { if (why) *why = w; return 1; };
    *p = Gemm16Plan{};
    p->epi = c.epi; p->f16 = c.f16;
    const int M = c.M, N = c.N, K = c.K, epi = c.epi;
    if (!(M > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 4 == 0 && c.lda % 8 == 0 && c.ldw % 8 == 0 && c.ldc % 4 == 0))
        return refuse("bad shape (M, N, K > 0; K % 64, N % 4, lda % 8, ldw % 8, ldc % 4)");
    if (n_cu < 8) return refuse("a device with fewer than 8 compute units");
    const int64_t blocks256 = (int64_t)cdiv(M, 256) * cdiv(N, 256);
    // shapes the LDS-DMA kernels take at all; then 256-wide N tiles unless that leaves too few workgroups for 256 CUs.  (From 192 tiles
    // on, round 4: the packed DistilBERT batch -- 18.8 k real tokens of [256, 128] -- is 74 x 3 = 222 tiles at N = 768, and only the
    // persistent kernel has the folded-LayerNorm epilogues.)
    const bool big = M >= 512 && N >= 128 && N % 8 == 0 && c.ldc % 8 == 0 && !sw.small;
    bool persistent = big && (sw.tile == 4 || (sw.tile == 0 && N % 256 == 0 && blocks256 >= 192));
    if (c.f16) {   // the decoder's big-batch prefill: the persistent kernel only (whatever the tile switch), epilogues 3 / 4 / 5 and the fp32-output head
        if (!(M >= 512 && N >= 256 && blocks256 >= 8)) return refuse("fp16: M, N below what the persistent kernel takes (M >= 512, N >= 256, 8 tiles)");
        if (!(epi >= BEPI_LNFOLD && epi <= BEPI_BIAS_F32)) return refuse("fp16: epilogue not built (3, 4, 5 or 6)");
        persistent = true;
    }
    if (epi < BEPI_BIAS || epi > BEPI_BIAS_F32 || (epi == BEPI_BIAS_F32 && !c.f16)) return refuse("bad epilogue");
    if (epi == BEPI_BIAS_F32 && !c.bias) return refuse("the fp32-output epilogue needs a bias");
    if (epi == BEPI_BIAS_RES && !c.res) return refuse("residual epilogue without residual");
    if (epi >= BEPI_LNFOLD && epi <= BEPI_RES_LN) {   // LayerNorm folded around the GEMM
        if (!c.bias) return refuse("the folded-LayerNorm epilogues need a bias / c2 vector");
        if (!(persistent && N % 256 == 0 && c.ldc % 8 == 0)) return refuse("the folded-LayerNorm epilogues exist on the persistent 256 x 256 kernel only (N % 256, ldc % 8)");
        if (epi == BEPI_RES_LN && !(c.res && c.rowstat && c.ln_g && c.ln_b))
            return refuse("RES_LN without residual / row statistics / gamma / beta (identity tables for a normalised residual)");
        if (epi != BEPI_RES_LN && !(c.rowstat && c.c1)) return refuse("LNFOLD without row statistics / c1");
    }
    const int cu8 = n_cu / 8 * 8;
    if (!c.f16 && !big) {
        p->family = G16_SMALL;
        p->tiles_n = cdiv(N, 128); p->n_tiles = cdiv(M, 128) * p->tiles_n;
        p->grid = p->n_tiles; p->block = 256;
    } else if (!c.f16 && sw.tile == 5 && epi != BEPI_BIAS_RES) {   // (prototype switch: plain epilogues only)
        p->family = G16_DUO;
        p->tiles_n = cdiv(N, 128); p->n_tiles = cdiv(M, 256) * p->tiles_n;
        p->grid = up8(p->n_tiles < 2 * cu8 ? p->n_tiles : 2 * cu8); p->block = 256;
        p->shmem = 2 * 256 * 128 + 128 * 128;               // 80 KB: two workgroups per CU
    } else if (persistent) {
        p->family = G16_PERSISTENT;
        p->phases = sw.phases == 1 ? 1 : sw.phases == 2 ? 2 : 4;
        p->tiles_n = cdiv(N, 256); p->n_tiles = cdiv(M, 256) * p->tiles_n;
        p->grid = up8(p->n_tiles < cu8 ? p->n_tiles : cu8);   // one persistent workgroup per CU (160 KB of LDS each)
        p->block = 512;
        p->shmem = 2 * (256 + 256) * 128 + 32768;           // two operand stages + the C stage: all 160 KB of the CU's LDS
        p->tail_mode = (sw.tail & 3) | (c.reverse && sw.reverse ? 4 : 0);
        p->half_tiles = gemm16_half_tiles(p->n_tiles, p->grid, p->tail_mode);
    } else {
        p->family = G16_RING;   // switch tile 1: 128 x 128 / 2: 256 x 128 / 3: 256 x 256 (tools/gemm_bf16_bench.py); else by the shape
        if (sw.tile == 1) { p->nt = 2; p->wmw = 1; }
        else if (sw.tile == 2) { p->nt = 2; p->wmw = 2; }
        else if (sw.tile == 3 || (N % 256 == 0 && blocks256 >= 512)) { p->nt = 4; p->wmw = 2; }
        else { p->nt = 2; p->wmw = 2; }
        const int BM = 128 * p->wmw, BN = 64 * p->nt, NS = (p->nt == 2 && p->wmw == 2) ? 3 : 2;
        const int ring = NS * (BM + BN) * 128, stage_c = BM * (BN * 2 + 16);
        p->tiles_n = cdiv(N, BN); p->n_tiles = cdiv(M, BM) * p->tiles_n;
        p->grid = p->n_tiles; p->block = 256 * p->wmw;
        p->shmem = ring > stage_c ? ring : stage_c;         // 64 KB .. 144 KB of the 160 KB LDS
    }
    return 0;
}

}  // namespace mgea
