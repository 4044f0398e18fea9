// What the 16-bit kernel families share (gemm16.hip, attn16.hip, rows16.hip): the vector types and X16<T> (bf16 / fp16 behind one
// set of kernels), the one-transcendental erf-GELU of the epilogues, the hidden LDS-DMA issue of the pipelined kernels and the
// half-wave sum.  The BEPI_* epilogue names are host-visible: gemm16_plan.h, through common.h.  Device code only.
#pragma once
#include "common.h"

namespace mgea {

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// erf-GELU for bf16 outputs with ONE transcendental.  With a = |x|: gelu(x) = max(x, 0) - 0.5 a erfc(a / sqrt 2), and
// erfc(a / sqrt 2) = 2^q(a) where q = log2(erfcx) - (a^2 / 2) log2 e is smooth: a degree-5 polynomial (weighted least squares on
// [0, 6.5], fitted and checked in fp32 against scipy's erf: |gelu error| < 1.5e-5 on [-12, 12], far below the 2^-9 rounding of the
// bf16 result; beyond 6.5 the clamped tail is < 2^-30).  11 instructions per element, v_exp_f32 the only quarter-rate one.  History:
// A&S 7.1.26 with a full-precision division and libm-style exp cost ~40 (14 us of a 40 us FC1 tile round); A&S 7.1.25 on
// v_rcp_f32 + v_exp_f32 12 with two transcendentals, still 28 of FC1's 169 us (measured by switching GELU off).
#define MGEA_GELU_D0 -1.585257735e-05f
#define MGEA_GELU_D1 -1.150631181e+00f
#define MGEA_GELU_D2 -4.612153958e-01f
#define MGEA_GELU_D3 -4.992833406e-02f
#define MGEA_GELU_D4 6.105210696e-03f
#define MGEA_GELU_D5 -3.249367875e-04f
#define MGEA_GELU_AMAX 6.505382387f
__device__ __forceinline__ float gelu_fast(float x) {
    const float a = fminf(fabsf(x), MGEA_GELU_AMAX);
    float q = fmaf(MGEA_GELU_D5, a, MGEA_GELU_D4);
    q = fmaf(q, a, MGEA_GELU_D3);
    q = fmaf(q, a, MGEA_GELU_D2);
    q = fmaf(q, a, MGEA_GELU_D1);
    q = fmaf(q, a, MGEA_GELU_D0);
    return fmaf(-0.5f * a, __builtin_amdgcn_exp2f(q), fmaxf(x, 0.f));
}
// Two elements with packed fp32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32: two results per instruction).  For epilogues only --
// beside MFMAs packed fp32 is slower than scalar (MI355X_MICROARCH.md).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_fast2(f32x2 x) {
    const f32x2 a = {fminf(fabsf(x[0]), MGEA_GELU_AMAX), fminf(fabsf(x[1]), MGEA_GELU_AMAX)};
    f32x2 q = __builtin_elementwise_fma((f32x2){MGEA_GELU_D5, MGEA_GELU_D5}, a, (f32x2){MGEA_GELU_D4, MGEA_GELU_D4});
    q = __builtin_elementwise_fma(q, a, (f32x2){MGEA_GELU_D3, MGEA_GELU_D3});
    q = __builtin_elementwise_fma(q, a, (f32x2){MGEA_GELU_D2, MGEA_GELU_D2});
    q = __builtin_elementwise_fma(q, a, (f32x2){MGEA_GELU_D1, MGEA_GELU_D1});
    q = __builtin_elementwise_fma(q, a, (f32x2){MGEA_GELU_D0, MGEA_GELU_D0});
    const f32x2 e = {__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])};
    const f32x2 pos = {fmaxf(x[0], 0.f), fmaxf(x[1], 0.f)};
    return __builtin_elementwise_fma(a * -0.5f, e, pos);
}

// One 1 KiB LDS-DMA piece (64 lanes x 16 B, LDS destination = wave-uniform byte address + 16 * lane) issued from inline
// asm, so that hipcc does not see it: seen through the builtin, ROCm 7.2 puts an s_waitcnt vmcnt(0) in front of the next
// ds_read of every phase (it cannot tell which LDS bytes a pending DMA writes) and the pipeline drains.  Hidden, none of the
// compiler's waits refer to it; every wait for these pieces is one of the hand-counted vmcnt of the kernel that issued them (the persistent GEMM has no other
// vector-memory instruction between its prologue and its epilogue).  M0 is compiler-reserved: saved and restored in the same
// statement (cdna_hip_programming.md section 5.7).
__device__ __forceinline__ void glds16_hidden(const void* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}

// Same, with a wave-uniform 64-bit base in SGPRs and a 32-bit byte offset per lane (no 64-bit vector address arithmetic).
__device__ __forceinline__ void glds16_hidden_s(const void* sbase, unsigned voff, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}

typedef unsigned long long u64x1;

// The two 16-bit storage types of the perf modes (bf16: DistilBERT, MGEA_DTYPE_BF16; fp16: the decoder's big-batch prefill,
// MGEA_DTYPE_F16) behind one set of kernels: vector types, the 16 x 16 x 32 MFMA, and a packed pair (one dword) <-> two fp32.
template <typename T> struct X16;
template <> struct X16<__bf16> {
    static constexpr bool is_bf16 = true;
    static constexpr float attn_rescale_log2 = 16.0f;   // flash attention, deferred rescale: p = 2^((s - m) kexp) <= 2^16 is far inside bf16's range
    typedef bf16x8 v8; typedef bf16x4 v4; typedef bf16x2 v2;
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x2 unpack(unsigned u) { return (f32x2){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }
};
template <> struct X16<_Float16> {
    static constexpr bool is_bf16 = false;
    static constexpr float attn_rescale_log2 = 15.0f;   // p <= 2^15: fp16 rounds every p from 65520 up to +inf (its largest finite value is 65504)
    typedef h16x8 v8; typedef h16x4 v4; typedef _Float16 v2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x2 unpack(unsigned u) {
        const v2 h = __builtin_bit_cast(v2, u);
        return (f32x2){(float)h[0], (float)h[1]};
    }
};

// Sum over the 32 lanes of a half wave (lanes 32 h .. 32 h + 31), result in all of them: four DPP row rotations (VALU speed) give
// the 16-lane sums, one ds_bpermute adds the neighbouring row.  (Five __shfl_xor steps = five trips through the LDS pipeline per
// value: 160 of them per tile made the statistics cost more than the LayerNorm kernel they replace.)
__device__ __forceinline__ float half_wave_sum(float v) {
#define MGEA_ROR_ADD(n) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (n), 0xf, 0xf, false))
    MGEA_ROR_ADD(1); MGEA_ROR_ADD(2); MGEA_ROR_ADD(4); MGEA_ROR_ADD(8);
#undef MGEA_ROR_ADD
    return v + __shfl_xor(v, 16, 64);
}

}  // namespace mgea
