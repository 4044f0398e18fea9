// Token sampler over a logits matrix [B, V]: replaces api_cache.py:169-178
//   logits / temperature -> additive -1e10 outside the top-k -> softmax -> multinomial(1)
// plus a build-defined nucleus (top-p) cut that the reference does not have, and the build's own row processors in front
// of it (repetition penalty, bias, grammar mask) and behind it (min-p, typical-p, epsilon and eta cutoff).
// One 256-thread workgroup per row; the row lives in registers (thread t owns logits t, t + 256, ...), nothing is sorted.  The file reads
// top down: the reductions and searches the stages share, the stages in calling order (each with its rule), the kernel, launch_sample.
// The sampler's scalars (temperature, top_k, top_p, seed, Philox stream; eos and budget for the fused tail) are read from the row's
// SamplerParams record in DEVICE memory when the caller passes the records: the captured decode graph then serves every request, whatever
// its seed (the reference's endpoint draws a fresh one per call, api_cache.py:204), and rows with different settings share one launch
// (workgroup b reads record b, so every setting stays block-uniform).
#include <cmath>
#include <type_traits>

#include "common.h"

namespace mgea {

__device__ __forceinline__ uint32_t fkey(float f) {  // larger float -> larger key
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {   // inverse of fkey
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += W0; k1 += W1;
    }
}

constexpr int SAMP_NT = 256, SAMP_NW = SAMP_NT / 64;   // threads / waves per row

__device__ __forceinline__ float block_sum_f(float v, float* red /* [SAMP_NW] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < SAMP_NW; ++w) t += red[w];          // fixed order: deterministic
    return t;
}

// LEAD = false: without the barrier in front of the write, for a `red` that no wave can still be reading (its first use in the kernel)
template <bool LEAD = true>
__device__ __forceinline__ float block_max_f(float v, float* red /* [SAMP_NW] */) {
    v = wave_max(v);
    if constexpr (LEAD) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < SAMP_NW; ++w) t = fmaxf(t, red[w]);
    return t;
}

// Whole-wave reductions on DPP alone (no LDS crossbar: a ds_bpermute round trip is ~100+ cycles, and the bisections below reduce once or
// twice per pass): butterfly inside each row of 16 lanes, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 (gfx9 DPP
// controls), the result read from lane 63 -- wave-uniform, in a scalar register.
#define MGEA_DPP(v, ctrl, rows) __builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rows, 0xF, true)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)MGEA_DPP(v, 0xB1, 0xF);    // quad_perm [1,0,3,2]
    v += (uint32_t)MGEA_DPP(v, 0x4E, 0xF);    // quad_perm [2,3,0,1]
    v += (uint32_t)MGEA_DPP(v, 0x141, 0xF);   // row_half_mirror
    v += (uint32_t)MGEA_DPP(v, 0x140, 0xF);   // row_mirror: every lane holds its row's sum
    v += (uint32_t)MGEA_DPP(v, 0x142, 0xA);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)MGEA_DPP(v, 0x143, 0xC);   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {   // rows not written by a masked step see 0: neutral for an unsigned maximum
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0xB1, 0xF));
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0x4E, 0xF));
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0x141, 0xF));
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0x140, 0xF));
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0x142, 0xA));
    v = umax32(v, (uint32_t)MGEA_DPP(v, 0x143, 0xC));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Boundary search shared by top-k (weights = 1, target = k) and top-p (weights = fixed-point mass): the largest key t
// with weight({key >= t, key >= floor_key}) >= target, i.e. the k-th largest logit / the logit at which the nucleus
// mass is reached; floor_key if even everything weighs less than the target.  Bit-by-bit bisection of the 32-bit
// order-preserving key over the thread's register-resident keys (0 = not a candidate): 32 counting passes, integer
// arithmetic only -> exact and deterministic.  Counts come from wave ballots (no reduction at all); masses are summed
// as two 20-bit halves in 32-bit lanes.  One barrier per pass (the cross-wave slots alternate with the pass parity).
// (The first version descended a radix tree through LDS histograms; with ~8k logits sharing a handful of exponent
// bytes its 64-bit LDS atomics serialised.)
template <bool MASS, int MAXE>
__device__ __forceinline__ uint32_t bisect_boundary(const uint32_t (&key)[MAXE], const uint32_t (&whi)[MAXE], const uint32_t (&wlo)[MAXE],
                                                    uint32_t floor_key, unsigned long long target, unsigned long long* red /* [2 * SAMP_NW] */,
                                                    unsigned long long* weight_at_boundary = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t prefix = 0u;
    unsigned long long at = ~0ull;   // weight({key >= prefix}): everything while prefix == 0
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        const uint32_t lim = cand > floor_key ? cand : floor_key;   // only keys >= floor_key are candidates
        unsigned long long mine;
        if (MASS) {
            uint32_t hi = 0u, lo = 0u;
#pragma unroll
            for (int j = 0; j < MAXE; ++j) {
                const bool in = key[j] >= lim;
                hi += in ? whi[j] : 0u;
                lo += in ? wlo[j] : 0u;
            }
            mine = ((unsigned long long)wave_sum_u32(hi) << 20) + wave_sum_u32(lo);
        } else {
            uint32_t cnt = 0u;
#pragma unroll
            for (int j = 0; j < MAXE; ++j) cnt += (uint32_t)__popcll(__ballot(key[j] >= lim));
            mine = cnt;
        }
        unsigned long long* slot = red + SAMP_NW * (bit & 1);
        if (lane == 0) slot[wave] = mine;
        __syncthreads();
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < SAMP_NW; ++w) tot += slot[w];
        if (tot >= target) { prefix = cand; at = tot; }
    }
    __syncthreads();   // the slots are reused by the caller
    if (weight_at_boundary) *weight_at_boundary = at;
    return prefix > floor_key ? prefix : floor_key;
}

// ---- top-k without a pass over the row per bit (round 4).  A wave issues one instruction per ~5 cycles when it is alone on its SIMD, as
// here, scalar ones included: the block-wide bisection is 32 x (36 compares + 72 scalar count instructions), ~12 us of the kernel's 21.
// (A first attempt kept those passes and only dropped their barrier -- every wave bisecting its own quarter, candidates merged at the end:
// 25 us, SLOWER; the passes themselves are the cost.)  Instead a PIVOT cuts the row down to a few dozen candidates first:
//   1. every lane takes the largest of its keys; every wave bisects ITS 64 lane maxima (one compare per pass) for the j-th largest,
//      j = ceil(k / 4); the pivot P is the smallest of the four.  At least 4 j >= k logits are >= P, so the k-th largest is >= P, and with
//      one logit in ~36 being a lane maximum the number of logits >= P is about k (k = 50: 60-70 of 8324);
//   2. one pass over the row writes the keys >= P into the wave's 64 LDS slots (ballot prefix; most ballots are empty);
//   3. after a barrier every wave bisects the <= 4 x 64 candidates (4 per lane) for the k-th largest of the row, and counts the
//      candidates at or above it -- that is every such logit of the row, so ties are seen exactly as before.
// A wave with more than 64 logits >= P (heavy ties, or fewer than j valid lanes in some wave) sends the block to the block-wide
// bisection.  Integer counts throughout: same boundary key either way.  top_k <= SAMP_KFAST takes this path (topk_from_pivot).
constexpr int SAMP_KFAST = 64;

// p (a probability, <= 1) as the 2^-40 fixed-point integer floor(p * 2^40), split as hi = bits 20.., lo = bits 0..19 -- the integers the
// mass sums are made of.  All float operations below are exact (powers of two, an integer part, a remainder), so this is the same integer
// as (unsigned long long)((double)p * 2^40) at a third of the instructions (no f64, no 64-bit conversion).
__device__ __forceinline__ void mass_fixed(float p, uint32_t& hi, uint32_t& lo) {
    const float t = p * 1048576.0f;
    hi = (uint32_t)t;
    lo = (uint32_t)((t - (float)hi) * 1048576.0f);
}
// a probability the caller passes (top_p, typical_p) as the same fixed point: what the mass bisections look for
__device__ __forceinline__ unsigned long long mass_target(float p) { return (unsigned long long)((double)p * 1099511627776.0); }

// The non-zero keys a wave holds lie in [lo, hi]: every boundary the bisections below look for does too, so the bits above the highest
// bit in which lo and hi differ are already known.  Returns that common prefix and the number of low bits left to decide (32: nothing
// known -- no non-zero key at all, or keys on both sides of the top bit).
template <int N>
__device__ __forceinline__ uint32_t wave_common_prefix(const uint32_t (&key)[N], int* nbits) {
    uint32_t hi = 0u, lo_inv = 0u;   // lo via the maximum of the complements
#pragma unroll
    for (int j = 0; j < N; ++j) {
        hi = hi > key[j] ? hi : key[j];
        const uint32_t c = key[j] != 0u ? ~key[j] : 0u;
        lo_inv = lo_inv > c ? lo_inv : c;
    }
    hi = wave_max_u32(hi);
    const uint32_t lo = ~wave_max_u32(lo_inv);   // 0xFFFFFFFF when there is no non-zero key
    const uint32_t diff = hi ^ lo;
    const int nb = (hi == 0u) ? 32 : 32 - __clz((int)diff);   // diff == 0: one distinct key, nothing left to decide (clz(0) = 32)
    *nbits = nb;
    return nb >= 32 ? 0u : (hi >> nb) << nb;
}

template <int N>
__device__ __forceinline__ uint32_t wave_kth_largest(const uint32_t (&key)[N], uint32_t k) {   // 0 when fewer than k keys are non-zero
    // (starting below the keys' common prefix, as wave_mass_boundary does, was measured here too: the two wave reductions cost more than
    // the ~10 passes of N compares they save -- top-k 50 at 12.2 us against 11.5)
    uint32_t prefix = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        uint32_t cnt = 0u;
#pragma unroll
        for (int j = 0; j < N; ++j) cnt += (uint32_t)__popcll(__ballot(key[j] >= cand));
        if (cnt >= k) prefix = cand;
    }
    return prefix;
}

// keys >= pivot (> 0) of this wave's registers -> slots[0, 64), zeros behind them; returns how many there were (may exceed 64)
template <int N>
__device__ __forceinline__ int wave_publish_ge(const uint32_t (&key)[N], uint32_t pivot, uint32_t* slots) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool up = key[j] >= pivot;
        const unsigned long long m = __ballot(up);
        if (m != 0ull) {   // wave-uniform, rarely taken
            const int pos = base + __popcll(m & below);
            if (up && pos < SAMP_KFAST) slots[pos] = key[j];
            base += __popcll(m);
        }
    }
    if (lane >= base) slots[lane] = 0u;   // SAMP_KFAST == 64: one lane per slot
    return base;
}

// ---- top-p without a top-k (or behind one larger than SAMP_KFAST): no count bounds the nucleus, so the candidates come from a mass
// histogram instead.  Bucket = floor((max - x) * scale), 256 of them over the row's own span below its maximum -- or over the 28
// units beyond which a probability rounds to 0 in the 2^-40 fixed point, if the row spans more -- non-increasing in the key, so the
// buckets are ordered slices of the sorted row.  (With a fixed 28-unit span a random-weight model's nearly flat rows -- all 8324 logits
// within ~2.5 units -- put hundreds of entries into the boundary bucket and every step fell back: configs[4]'s sampler 32 -> 37.6 us.)
//   1. one pass adds every entry's fixed-point mass to its bucket (64-bit LDS atomics: integer sums, order-free);
//   2. every wave scans the 256 buckets (4 per lane) for the first one at which the running mass reaches the target: the nucleus
//      boundary lies in it, and everything in the buckets before it is kept;
//   3. one pass writes that bucket's keys into the wave's 64 LDS slots; every wave bisects those <= 4 x 64 candidates for the largest
//      key at which (mass before the bucket + mass of the candidates at or above it) reaches the target.
// Same integers as the block-wide bisection -> same boundary key.  More than 64 candidates in a wave: the block-wide bisection
// (topp_from_histogram).
constexpr float SAMP_HSPAN = 28.0f;

__device__ __forceinline__ int mass_bucket(float mx, float x, float scale) {
    const int b = (int)((mx - x) * scale);   // v_cvt_i32_f32: NaN -> 0, +inf saturates
    return (unsigned)b > 255u ? 255 : b;
}

// first bucket whose inclusive running mass reaches `target`, and the mass before it; -1 when the whole row weighs less
__device__ __forceinline__ int wave_find_bucket(const unsigned long long* hist /* [256] in LDS */, unsigned long long target,
                                                unsigned long long* before) {
    const int lane = threadIdx.x & 63;
    unsigned long long h[4], c[5];
    c[0] = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) { h[i] = hist[4 * lane + i]; c[i + 1] = c[i] + h[i]; }
    unsigned long long inc = c[4];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    const unsigned long long excl = inc - c[4];
    const unsigned long long hit = __ballot(inc >= target);
    if (hit == 0ull) { *before = 0ull; return -1; }
    const int L = __ffsll((long long)hit) - 1;
    int i = 0;
#pragma unroll
    for (int q = 3; q >= 0; --q) i = excl + c[q + 1] >= target ? q : i;   // first of my four that reaches it
    unsigned long long bef = excl + (i == 0 ? c[0] : i == 1 ? c[1] : i == 2 ? c[2] : c[3]);
    const int b = __shfl(4 * lane + i, L, 64);
    *before = __shfl(bef, L, 64);
    return b;
}

// the mass bisection of bisect_boundary<true> over candidates a single wave holds (R per lane): same integers, same boundary
template <int R>
__device__ __forceinline__ uint32_t wave_mass_boundary(const uint32_t (&key)[R], const uint32_t (&whi)[R], const uint32_t (&wlo)[R],
                                                       uint32_t floor_key, unsigned long long target) {
    // candidates that count: key >= floor_key and non-zero (the others carry no mass: whi = wlo = 0)
    uint32_t live[R];
    uint32_t hi = 0u, lo = 0u;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        live[j] = (key[j] >= floor_key && (whi[j] | wlo[j]) != 0u) ? key[j] : 0u;
        hi += live[j] != 0u ? whi[j] : 0u;
        lo += live[j] != 0u ? wlo[j] : 0u;
    }
    const unsigned long long all = ((unsigned long long)wave_sum_u32(hi) << 20) + wave_sum_u32(lo);
    if (all < target) return floor_key;   // even everything weighs less: the bisection would end at prefix 0
    int nbits;
    uint32_t prefix = wave_common_prefix<R>(live, &nbits);   // mass({key >= lowest live key}) = all >= target: the boundary is among them
    for (int bit = nbits - 1; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        hi = 0u; lo = 0u;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const bool in = live[j] >= cand;
            hi += in ? whi[j] : 0u;
            lo += in ? wlo[j] : 0u;
        }
        const unsigned long long tot = ((unsigned long long)wave_sum_u32(hi) << 20) + wave_sum_u32(lo);
        if (tot >= target) prefix = cand;
    }
    return prefix > floor_key ? prefix : floor_key;
}

// the scored form's three LDS words: the raw row's maximum, the log of its exp-sum, the final id's mass
__device__ __forceinline__ float* score_lds() {
    __shared__ float s[3];
    return s;
}
// the argument of type T among a kernel's optional trailing arguments (ScoreArgs, GrammarArgs, TruncArgs), T{} when it was not passed
template <typename T>
__device__ __forceinline__ T extra_arg() { return T{}; }
template <typename T, typename A, typename... R>
__device__ __forceinline__ T extra_arg(const A& a, const R&... r) {
    if constexpr (std::is_same_v<T, A>) return a;
    else return extra_arg<T>(r...);
}

// ---- the stages of sample_kernel, in calling order.  Thread t holds logit t + SAMP_NT * j in slot j of x (the processed logit), key
// (its order-preserving key; 0 = not kept, below every real key) and whi / wlo (its fixed-point mass while a mass bisection runs).
// The workgroup's LDS that every instantiation has, by owner (declared in the kernel: the names fix the layout; the feature-owned
// objects are passed to their stages by name).  Reused on purpose, each time behind the barrier its stage names: red64 by every
// bisect_boundary; cand and fit by the top-k pivot path, then by the top-p histogram path; tie by the pivot exchange, then the tie
// trim; redf by the row maximum and every block_sum_f / block_max_f behind it.
struct SampleLds {
    unsigned long long* red64;   // [2 * SAMP_NW] selection: bisect_boundary's cross-wave slots
    uint32_t* cand;              // [SAMP_NW * SAMP_KFAST] every wave's published candidates
    unsigned long long* hist;    // [SAMP_NT] top-p's mass histogram
    int *tie, *fit;              // [SAMP_NW] each
    float *redf, *low;           // [SAMP_NW] each: float reductions; low rides on top-p's block_sum_f
    float* scan;                 // [SAMP_NW] final distribution: the waves' totals
    int *thread, *choice;        // draw: the last thread whose prefix is <= the target, the id drawn
};
__device__ __forceinline__ bool kept(uint32_t key, uint32_t keep_key) { return key != 0u && key >= keep_key; }
// the thread's share of sum exp(x - mx) over the kept set, registers in ascending order
// (the predicate is spelt out here: through kept() its compares are shared with the later stages', and of the 28 instantiations
// <56, false, true, ScoreArgs> then spills 20 bytes per lane -- the wide forms sit at 240-250 of 256 AGPRs)
template <int MAXE> __device__ __forceinline__ float kept_mass(const float (&x)[MAXE], const uint32_t (&key)[MAXE], uint32_t keep_key, float mx) {
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) z += (key[j] != 0u && key[j] >= keep_key) ? __expf(x[j] - mx) : 0.f;
    return z;
}
// H = -sum p log p over {key != 0}, p = exp(x - mx) / Z with invZ = 1 / Z and logZ = log Z
template <int MAXE> __device__ __forceinline__ float kept_entropy(const float (&x)[MAXE], const uint32_t (&key)[MAXE], float mx, float invZ, float logZ,
        float* redf) {
    float h = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const float pj = key[j] != 0u ? __expf(x[j] - mx) * invZ : 0.f;
        h += pj > 0.f ? pj * ((x[j] - mx) - logZ) : 0.f;   // p = 0 adds nothing (never 0 * -inf)
    }
    return -block_sum_f(h, redf);
}
// the step index of row b: per row from device memory, or the call's (Philox counter word 1; what min_new and forced ids are indexed by)
__device__ __forceinline__ int32_t step_of(const int32_t* row_step, int64_t step_host, int b) {
    return row_step ? row_step[b] : (int32_t)step_host;
}
// the row's loop state, read by thread 0 at kernel start for the fused tail
struct RowLoop { int step, fed, len, done; RowStops stops; };
// GRAMMAR (the instantiations with a GrammarArgs argument, PENALTY and BIAS ones only; common.h): a row whose state s is >= 0 and which
// is not finished loses every id whose class s bans, x[i] = -inf, after the bias and before the EOS ban; its thread 0 then stores the
// state behind the id the step commits.  The state is one scalar load at kernel start; -1 = no grammar on this row (or the row is
// finished): such a row skips all of it (block-uniform) and computes what the BIAS form computes.
__device__ __forceinline__ int grammar_row_state(const GrammarArgs& gr, int b) {
    int gstate = gr.state_in[b];
    if (gstate >= gr.n_state || (gr.done && gr.done[b])) gstate = -1;
    return gstate;
}
// SCORED: the id this step must take, requested at kernel start and consumed after the draw (< 0: the draw decides)
__device__ __forceinline__ int forced_id(const ScoreArgs& sc, const int32_t* row_step, int64_t step_host, int b) {
    int forced = -1;
    if (sc.forced) {
        const int step = step_of(row_step, step_host, b);
        if (sc.forced_stride == 0) forced = sc.forced[b];
        else if (step >= 0 && step < sc.forced_stride) forced = sc.forced[(int64_t)b * sc.forced_stride + step];
    }
    return forced;
}
// ---- load.  The whole row is requested at once (a rolled loop pays one ~1 us round trip per pass: the row was just written by the
// head kernel and sits in another XCD's L2 / the Infinity Cache); it is read from memory once and never goes through LDS.
template <int MAXE> __device__ __forceinline__ void load_row(const float* lg, int V, float (&x)[MAXE]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const int i = tid + SAMP_NT * j;
        x[j] = i < V ? lg[i] : -INFINITY;
    }
}
// BIAS: the row's bias (V floats per row, row b at b * V; read by the rows whose record has bias_on) travels in the same batch of loads
// (nothing above waits for the logits yet); block-uniform
template <int MAXE> __device__ __forceinline__ void load_bias(const float* br, int V, bool biased, float (&bz)[MAXE]) {
    // (the condition stays outside the unrolled loads: selected per element, every load gets a branch and a wait of its own)
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) bz[j] = 0.f;
    if (biased) {
#pragma unroll
        for (int j = 0; j < MAXE; ++j) {
            const int i = tid + SAMP_NT * j;
            bz[j] = i < V ? br[i] : 0.f;
        }
    }
}
// GRAMMAR: so do the classes of the thread's ids (class_of, shared by all rows, L2-resident: no dependent round trip), and the state's
// row of the allow bitmask (<= 128 words) on its way to LDS next to the presence words; block-uniform
template <int MAXE> __device__ __forceinline__ void load_classes(const GrammarArgs& gr, int V, int gstate, int (&gcls)[MAXE], uint32_t* s_gram) {
    const int tid = threadIdx.x;
    if (gstate >= 0) {
#pragma unroll
        for (int j = 0; j < MAXE; ++j) {
            const int i = tid + SAMP_NT * j;
            gcls[j] = i < V ? gr.class_of[i] : 0;
        }
        if (tid < gr.words) s_gram[tid] = gr.allow[(int64_t)gstate * gr.words + tid];   // words <= 128 < NT; read after the penalty's barrier
    }
}
// ---- SCORED: the raw log-probability of the row's id is x_id - m - log sum_i exp(x_i - m) over the RAW row, m = its maximum.  Both are
// reduced here, right after the load, while x still holds what the head wrote (no second copy of the row); fixed reduction order, fp32;
// kept in score_lds() for thread 0's use at the end, where x_id is re-read from the row.
template <int MAXE> __device__ __forceinline__ void raw_logsumexp(const float (&x)[MAXE], float* s_rawm, float* s_raws) {
    const int tid = threadIdx.x;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) m = fmaxf(m, x[j]);
    m = block_max_f<false>(m, s_rawm);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) s += __expf(x[j] - m);   // the padding beyond V is -inf: exactly 0
    s = wave_sum(s);
    if ((tid & 63) == 0) s_raws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        score_lds()[0] = m;
        score_lds()[1] = logf((s_raws[0] + s_raws[1]) + (s_raws[2] + s_raws[3]));   // fixed order: deterministic
    }
    static_assert(SAMP_NW == 4, "the log-sum merges four wave sums");
}
// ---- PENALTY (HF RepetitionPenaltyLogitsProcessor): before everything else, every logit whose id is set in the row's presence bitmap
// (presence_words(V) words per row, updated by the fused tail) becomes x < 0 ? x * p : x / p (one correctly rounded fp32 operation).
// The row's bitmap words are staged in LDS first (<= 448 words: two per thread at most); the barrier behind them also publishes
// load_classes' grammar words.
__device__ __forceinline__ void stage_presence(const uint32_t* presence, int V, int b, uint32_t* s_pres) {
    const int tid = threadIdx.x, nw = presence_words(V);   // <= MAXE * NT / 32
    for (int w = tid; w < nw; w += SAMP_NT) s_pres[w] = presence[(int64_t)b * nw + w];
    __syncthreads();
}
// GRAMMAR: every thread folds its ids' verdicts into one 64-bit word (MAXE <= 64), bit j: the row's state bans logit tid + NT * j -- all
// that stays live until the mask is applied
template <int MAXE> __device__ __forceinline__ unsigned long long grammar_verdicts(const GrammarArgs& gr, const int (&gcls)[MAXE], const uint32_t* s_gram) {
    unsigned long long gban = 0ull;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const uint32_t c = (uint32_t)gcls[j] < (uint32_t)gr.n_class ? (uint32_t)gcls[j] : 0u;   // (set_grammar checked the table: never taken)
        gban |= (unsigned long long)(((s_gram[c >> 5] >> (c & 31)) & 1u) ^ 1u) << j;
    }
    return gban;
}
template <int MAXE> __device__ __forceinline__ void apply_penalty(float (&x)[MAXE], int V, float pen, const uint32_t* s_pres) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const int i = tid + SAMP_NT * j;
        if (i < V && ((s_pres[i >> 5] >> (i & 31)) & 1u)) x[j] = x[j] < 0.f ? x[j] * pen : x[j] / pen;
    }
}
// ---- BIAS (HF sequence_bias / suppress_tokens, OpenAI logit_bias -- build-defined, the reference has none): after the penalty and
// before everything else, a row whose record says so adds its fp32 bias row, x[i] += bias[i] (-inf = the id is banned); then the
// grammar's mask; then a row that has produced fewer than its record's min_new ids has x[eos_id] = -inf.  A banned entry is an ordinary
// logit from there on: its key is the smallest a real entry can have, exp(-inf - max) is exactly 0, so it carries no mass, is never
// drawn, and may sit among the top_k kept when fewer than top_k ids are admissible.  A row without a bias is not touched (no + 0).
template <int MAXE> __device__ __forceinline__ void add_bias(float (&x)[MAXE], const float (&bz)[MAXE]) {
#pragma unroll
    for (int j = 0; j < MAXE; ++j) x[j] += bz[j];
}
template <int MAXE> __device__ __forceinline__ void ban_classes(float (&x)[MAXE], unsigned long long gban) {
#pragma unroll
    for (int j = 0; j < MAXE; ++j)
        if ((gban >> j) & 1ull) x[j] = -INFINITY;
}
template <int MAXE> __device__ __forceinline__ void ban_id(float (&x)[MAXE], int id) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAXE; ++j)
        if (tid + SAMP_NT * j == id) x[j] = -INFINITY;
}
// ---- temperature and row maximum: logits / temperature (api_cache.py:170; x / 1 is x), then the maximum of the processed row
template <int MAXE> __device__ __forceinline__ float temper_and_max(float (&x)[MAXE], float temperature, bool divide, float* redf) {
    float mx = -INFINITY;
    if (divide) {
#pragma unroll
        for (int j = 0; j < MAXE; ++j) x[j] = x[j] / temperature;
    }
#pragma unroll
    for (int j = 0; j < MAXE; ++j) mx = fmaxf(mx, x[j]);
    return block_max_f<false>(mx, redf);
}
template <int MAXE> __device__ __forceinline__ void make_keys(const float (&x)[MAXE], int V, uint32_t (&key)[MAXE], uint32_t (&whi)[MAXE], uint32_t (&wlo)[MAXE]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        key[j] = (tid + SAMP_NT * j < V) ? fkey(x[j]) : 0u;   // 0 = below every candidate
        whi[j] = wlo[j] = 0u;
    }
}
// ---- top-k: the exact k-th largest logit by bit-wise bisection of order-preserving uint keys (integer counts -> deterministic), over a
// pivot-selected candidate list for top_k <= 64, over the registers otherwise; kept = {logit > k-th} plus as many of the entries EQUAL
// to the k-th as it takes to keep exactly k, lowest ids first (topk + scatter_ of api_cache.py:172-175 keeps exactly top_k entries;
// which of several tied ones torch keeps is unspecified, lowest-id is this build's rule).  exp(-1e10) underflows to exactly 0 in fp32,
// so "mask then softmax" == "softmax over kept".
// The pivot path ("top-k without a pass over the row per bit" above).  True: keep_key is the k-th largest, n_ge the entries at or above
// it, cand this lane's share of the candidates (all waves hold the same list) and cand_cover says that they contain every entry >=
// keep_key (no ties beyond top_k).  False: the block-wide bisection decides.
template <int MAXE> __device__ __forceinline__ bool topk_from_pivot(const uint32_t (&key)[MAXE], int top_k, const SampleLds& l, uint32_t (&cand)[SAMP_NW],
        uint32_t& keep_key, unsigned long long& n_ge, bool& cand_cover) {
    constexpr int NW = SAMP_NW; const int tid = threadIdx.x;
    uint32_t lm[1] = {key[0]};
#pragma unroll
    for (int j = 1; j < MAXE; ++j) lm[0] = lm[0] > key[j] ? lm[0] : key[j];
    const uint32_t piv_w = wave_kth_largest<1>(lm, (uint32_t)((top_k + NW - 1) / NW));
    if ((tid & 63) == 0) l.tie[tid >> 6] = (int)piv_w;
    __syncthreads();
    uint32_t pivot = (uint32_t)l.tie[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) pivot = pivot < (uint32_t)l.tie[w] ? pivot : (uint32_t)l.tie[w];
    if (pivot != 0u) {   // block-uniform; 0: some wave has fewer than j valid lanes (a tiny vocabulary)
        const int n_w = wave_publish_ge<MAXE>(key, pivot, l.cand + (tid >> 6) * SAMP_KFAST);
        if ((tid & 63) == 0) l.fit[tid >> 6] = n_w;
    }
    __syncthreads();
    bool fast = pivot != 0u;
    if (fast) {
#pragma unroll
        for (int w = 0; w < NW; ++w) fast = fast && l.fit[w] <= SAMP_KFAST;
    }
    if (fast) {
#pragma unroll
        for (int r = 0; r < NW; ++r) cand[r] = l.cand[(tid & 63) + 64 * r];
        keep_key = wave_kth_largest<NW>(cand, (uint32_t)top_k);   // >= pivot: at least top_k candidates exist
#pragma unroll
        for (int r = 0; r < NW; ++r) n_ge += (unsigned long long)__popcll(__ballot(cand[r] >= keep_key));
        cand_cover = n_ge == (unsigned long long)top_k;   // more: ties, trimmed below in the registers only
    }
    return fast;
}
// several logits equal the k-th largest: keep exactly top_k entries, the tied ones by ascending id (id = tid + NT j, so the order is
// j-major, thread-minor).  Rare (exact fp32 ties): block-uniform branch.
template <int MAXE> __device__ __forceinline__ void topk_trim_ties(uint32_t (&key)[MAXE], uint32_t keep_key, int top_k, int* s_tie) {
    constexpr int NW = SAMP_NW; const int tid = threadIdx.x;
    uint32_t n_gt = 0u;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) n_gt += (uint32_t)__popcll(__ballot(key[j] > keep_key));
    if ((tid & 63) == 0) s_tie[tid >> 6] = (int)n_gt;
    __syncthreads();
    int n_gt_all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) n_gt_all += s_tie[w];
    const int need = top_k - n_gt_all;   // >= 1 tied entries survive
    __syncthreads();
    int seen = 0;   // tied entries with a lower id than this pass's (block-uniform)
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const bool tie = key[j] == keep_key;
        const unsigned long long bal = __ballot(tie);
        if ((tid & 63) == 0) s_tie[tid >> 6] = __popcll(bal);
        __syncthreads();
        int before = seen + __popcll(bal & ((1ull << (tid & 63)) - 1ull));
        for (int w = 0; w < NW; ++w) {
            if (w < (tid >> 6)) before += s_tie[w];
            seen += s_tie[w];
        }
        if (tie && before >= need) key[j] = 0u;   // 0 = not a candidate: below every kept key
        __syncthreads();
    }
}
template <int MAXE> __device__ __forceinline__ uint32_t topk_stage(uint32_t (&key)[MAXE], const uint32_t (&whi)[MAXE], const uint32_t (&wlo)[MAXE], int top_k,
        int wave_select, const SampleLds& l, uint32_t (&cand)[SAMP_NW], bool& cand_cover) {
    uint32_t keep_key = 0u;
    unsigned long long n_ge = 0;
    bool fast = false;
    if (wave_select && top_k <= SAMP_KFAST) fast = topk_from_pivot<MAXE>(key, top_k, l, cand, keep_key, n_ge, cand_cover);
    if (!fast) keep_key = bisect_boundary<false, MAXE>(key, whi, wlo, 0u, (unsigned long long)top_k, l.red64, &n_ge);
    if (n_ge > (unsigned long long)top_k) topk_trim_ties<MAXE>(key, keep_key, top_k, l.tie);
    return keep_key;
}
// ---- top-p: the nucleus {i : mass of strictly larger logits < top_p} by the same bisection over fixed-point (2^-40) probability masses
// (64-bit integer sums -> deterministic), over the candidates of the top-k path or of a mass histogram ("top-p without a top-k"
// above), over the registers otherwise; kept = {logit >= boundary}.
// The kept set is among the candidates every wave already holds: the nucleus boundary without a barrier per bit.  The masses are the
// same integers (same x, mx, invZ), so the boundary is the one the block-wide bisection finds.
__device__ __forceinline__ uint32_t topp_from_candidates(const uint32_t (&cand)[SAMP_NW], uint32_t keep_key, float mx, float invZ, unsigned long long target)
        {
    uint32_t chi[SAMP_NW], clo[SAMP_NW];
#pragma unroll
    for (int r = 0; r < SAMP_NW; ++r) {
        chi[r] = clo[r] = 0u;
        if (kept(cand[r], keep_key)) mass_fixed(__expf(funkey(cand[r]) - mx) * invZ, chi[r], clo[r]);
    }
    return wave_mass_boundary<SAMP_NW>(cand, chi, clo, keep_key, target);
}
// The histogram path; whi / wlo hold the kept entries' masses.  True: keep_key is settled; false: the block-wide bisection decides.
template <int MAXE> __device__ __forceinline__ bool topp_from_histogram(const float (&x)[MAXE], const uint32_t (&key)[MAXE], const uint32_t (&whi)[MAXE],
        const uint32_t (&wlo)[MAXE], float mx, float hscale, float invZ, unsigned long long target, const SampleLds& l, uint32_t (&cand)[SAMP_NW], uint32_t&
        keep_key) {
    constexpr int NW = SAMP_NW; const int tid = threadIdx.x;
    bool done = false;
    l.hist[tid] = 0ull;   // NT == 256 buckets
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const unsigned long long w = ((unsigned long long)whi[j] << 20) + wlo[j];
        if (w != 0ull) atomicAdd(&l.hist[mass_bucket(mx, x[j], hscale)], w);
    }
    __syncthreads();
    unsigned long long before = 0ull;
    const int bstar = wave_find_bucket(l.hist, target, &before);   // the same in every wave
    if (bstar < 0) {
        done = true;   // even everything weighs less than the target: keep all of it (keep_key stays the floor)
    } else {
        uint32_t inb[MAXE];   // the keys of that bucket (0 elsewhere)
#pragma unroll
        for (int j = 0; j < MAXE; ++j) inb[j] = ((whi[j] | wlo[j]) != 0u && mass_bucket(mx, x[j], hscale) == bstar) ? key[j] : 0u;
        const int n_w = wave_publish_ge<MAXE>(inb, 1u, l.cand + (tid >> 6) * SAMP_KFAST);
        if ((tid & 63) == 0) l.fit[tid >> 6] = n_w;
        __syncthreads();
        bool fits = true;
#pragma unroll
        for (int w = 0; w < NW; ++w) fits = fits && l.fit[w] <= SAMP_KFAST;
        if (fits) {
            uint32_t chi[NW], clo[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) {
                cand[r] = l.cand[(tid & 63) + 64 * r];
                chi[r] = clo[r] = 0u;
                if (cand[r] != 0u) mass_fixed(__expf(funkey(cand[r]) - mx) * invZ, chi[r], clo[r]);
            }
            keep_key = wave_mass_boundary<NW>(cand, chi, clo, keep_key, target - before);
            done = true;
        }
        __syncthreads();   // fit / cand / red64 are reused by the fallback
    }
    return done;
}
template <int MAXE> __device__ __forceinline__ uint32_t topp_stage(const float (&x)[MAXE], const uint32_t (&key)[MAXE], uint32_t (&whi)[MAXE], uint32_t
        (&wlo)[MAXE], float mx, float top_p, uint32_t keep_key, uint32_t (&cand)[SAMP_NW], bool cand_cover, int wave_select, const SampleLds& l) {
    constexpr int NW = SAMP_NW; const int tid = threadIdx.x;
    float lowest = mx;   // the smallest kept logit within SAMP_HSPAN of the maximum (the histogram's span)
    const float z = kept_mass<MAXE>(x, key, keep_key, mx);
    if (!cand_cover) {   // block-uniform: only the histogram path needs the span
#pragma unroll
        for (int j = 0; j < MAXE; ++j) lowest = (kept(key[j], keep_key) && x[j] >= mx - SAMP_HSPAN) ? fminf(lowest, x[j]) : lowest;
        lowest = -wave_max(-lowest);
        if ((tid & 63) == 0) l.low[tid >> 6] = lowest;   // rides on block_sum_f's barriers
    }
    const float invZ = 1.0f / block_sum_f(z, l.redf);
    if (!cand_cover) {
#pragma unroll
        for (int w = 0; w < NW; ++w) lowest = fminf(lowest, l.low[w]);
    }
    const float hscale = 255.99f / (mx - lowest);   // a one-value row: inf, every entry in bucket 0 (NaN -> 0) and the fallback below
    const unsigned long long target = mass_target(top_p);
    if (cand_cover) return topp_from_candidates(cand, keep_key, mx, invZ, target);
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        if (kept(key[j], keep_key)) mass_fixed(__expf(x[j] - mx) * invZ, whi[j], wlo[j]);   // hi <= 2^20: 64 lanes x MAXE of them stay below 2^32
    }
    const bool done = wave_select && topp_from_histogram<MAXE>(x, key, whi, wlo, mx, hscale, invZ, target, l, cand, keep_key);
    if (!done) keep_key = bisect_boundary<true, MAXE>(key, whi, wlo, keep_key, target, l.red64);
    return keep_key;
}
// ---- TRUNC (the instantiations with a TruncArgs argument, PENALTY and BIAS ones only; HF MinP / Typical / Epsilon / Eta warpers --
// build-defined, the reference has none; the rule: include/mgea.h, mgea_row_truncation): behind top-k and top-p a row whose record
// switches them on applies min-p, typical-p, the epsilon and the eta cutoff, in this order, each over the softmax of what is kept so
// far.  Every stage works on the registers the row already occupies (key, whi, wlo), so the wide instantiation stays without scratch.
// The kept set is {j : key[j] != 0} in all of them: a stage removes an entry by clearing its key.
// min-p: p_i < min_p * max(p) <=> exp(x_i - mx) < min_p (the normaliser cancels; mx is kept so far, and stays: 1 >= min_p)
template <int MAXE> __device__ __forceinline__ void trunc_min_p(const float (&x)[MAXE], uint32_t (&key)[MAXE], float mx, float min_p) {
#pragma unroll
    for (int j = 0; j < MAXE; ++j) key[j] = (key[j] != 0u && __expf(x[j] - mx) < min_p) ? 0u : key[j];
}
// typical-p: a band around the entropy, not a threshold.  The entries' keys become the order-preserving keys of -d_i, d_i =
// |(-log p_i) - H|, and their fixed-point masses go into whi / wlo, so the smallest d* that holds the mass is the mass boundary under
// that key, found by the bisection of top-p.  The row's maximum may have left: returns the kept set's own maximum.
template <int MAXE> __device__ __forceinline__ float trunc_typical(const float (&x)[MAXE], uint32_t (&key)[MAXE], uint32_t (&whi)[MAXE], uint32_t
        (&wlo)[MAXE], float mx, float typical_p, const SampleLds& l) {
    const float z = block_sum_f(kept_mass<MAXE>(x, key, 0u, mx), l.redf);
    const float invZ = 1.0f / z, logZ = __logf(z);
    const float H = kept_entropy<MAXE>(x, key, mx, invZ, logZ, l.redf);
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        whi[j] = wlo[j] = 0u;
        if (key[j] != 0u) {
            const float nlp = logZ - (x[j] - mx);   // -log p_i; +inf for a banned id, whose d is +inf
            key[j] = fkey(-fabsf(nlp - H));         // >= fkey(-inf) > 0: still "kept"
            mass_fixed(__expf(x[j] - mx) * invZ, whi[j], wlo[j]);
        }
    }
    const uint32_t band = bisect_boundary<true, MAXE>(key, whi, wlo, 0u, mass_target(typical_p), l.red64);   // 0: even everything weighs less
#pragma unroll
    for (int j = 0; j < MAXE; ++j) key[j] = key[j] >= band ? key[j] : 0u;
    float m2 = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) m2 = key[j] != 0u ? fmaxf(m2, x[j]) : m2;
    return block_max_f(m2, l.redf);
}
// the two probability floors: p_i < floor leaves, but the largest remaining logit stays (lowest id among equals).  The epsilon cutoff's
// floor is `cut`; ETA: eta' = min(eta, sqrt(eta) * exp(-H)), H the entropy of the current distribution.
template <int MAXE> __device__ __forceinline__ void trunc_floor(const float (&x)[MAXE], uint32_t (&key)[MAXE], float mx, float cut, bool eta, const SampleLds&
        l, int* s_first) {
    constexpr int NT = SAMP_NT; const int tid = threadIdx.x;
    const float z = block_sum_f(kept_mass<MAXE>(x, key, 0u, mx), l.redf);
    const float invZ = 1.0f / z;
    float floor_p = cut;
    if (eta) floor_p = fminf(cut, sqrtf(cut) * __expf(-kept_entropy<MAXE>(x, key, mx, invZ, __logf(z), l.redf)));
    // even the maximum (exp(0) / Z) is below the floor: it alone stays, the lowest id of its equals (block-uniform, rare)
    const bool none = invZ < floor_p;
    int first = -1;
    if (none) {
        int mine = 0x7fffffff;
#pragma unroll
        for (int j = MAXE - 1; j >= 0; --j) mine = (key[j] != 0u && x[j] == mx) ? j : mine;   // the thread's lowest
        mine = mine != 0x7fffffff ? tid + NT * mine : mine;
        if (tid == 0) *s_first = 0x7fffffff;
        __syncthreads();
        if (mine != 0x7fffffff) atomicMin(s_first, mine);
        __syncthreads();
        first = *s_first;
        __syncthreads();   // s_first may be rewritten by the next stage
    }
    // (the survivor as (owner thread, register index): one compare per thread and a uniform one per register -- spelt as
    // tid + NT * j == first, the 56 ids are hoisted out of the stage loop and the wide instantiation spills)
    const bool owner = first >= 0 && tid == (first & (NT - 1));
    const int fj = first >= 0 ? first / NT : -1;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        const bool out = none ? !(owner && j == fj) : __expf(x[j] - mx) * invZ < floor_p;
        key[j] = out ? 0u : key[j];
    }
}
// The record is block-uniform; a row that switches nothing on, and a top_k == 1 row, go straight to the final distribution with the
// keys they have.
template <int MAXE> __device__ __forceinline__ void truncate_stage(const float (&x)[MAXE], uint32_t (&key)[MAXE], uint32_t (&whi)[MAXE], uint32_t
        (&wlo)[MAXE], float& mx, uint32_t& keep_key, int top_k, const mgea_row_truncation tr, const SampleLds& l, int* s_first) {
    const bool typical_on = tr.typical_p > 0.f && tr.typical_p < 1.f;
    if (top_k != 1 && (tr.min_p > 0.f || typical_on || tr.epsilon_cutoff > 0.f || tr.eta_cutoff > 0.f)) {
        // from here on the kept set is {j : key[j] != 0}: the threshold goes into the keys, so that a stage removes an entry by
        // clearing its key and typical-p may put its own key there
#pragma unroll
        for (int j = 0; j < MAXE; ++j) key[j] = key[j] >= keep_key ? key[j] : 0u;
        keep_key = 0u;
        if (tr.min_p > 0.f) trunc_min_p<MAXE>(x, key, mx, tr.min_p);
        if (typical_on) mx = trunc_typical<MAXE>(x, key, whi, wlo, mx, tr.typical_p, l);
        for (int stage = 0; stage < 2; ++stage) {
            const float cut = stage == 0 ? tr.epsilon_cutoff : tr.eta_cutoff;
            if (!(cut > 0.f)) continue;   // block-uniform
            trunc_floor<MAXE>(x, key, mx, cut, stage == 1, l, s_first);
        }
    }
}
// ---- final distribution over the kept set, e = exp(x - mx), and its exclusive prefix in CDF order = thread-major (t, then t + NT,
// ...): any fixed order gives the same distribution.  Returns the thread's mass.
template <int MAXE> __device__ __forceinline__ float kept_distribution(const float (&x)[MAXE], const uint32_t (&key)[MAXE], uint32_t keep_key, float mx, float
        (&e)[MAXE]) {
    float loc = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; ++j) {
        e[j] = kept(key[j], keep_key) ? __expf(x[j] - mx) : 0.f;
        loc += e[j];
    }
    return loc;
}
// exclusive prefix of the per-thread masses in thread order: a fixed tree (wave scan, then the wave totals left to right) ->
// deterministic.  The draw's two LDS words are cleared under the same barrier.
__device__ __forceinline__ float exclusive_scan(float loc, const SampleLds& l, float* total_out) {
    const int tid = threadIdx.x;
    float inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += up;
    }
    if ((tid & 63) == 63) l.scan[tid >> 6] = inc;
    if (tid == 0) { *l.thread = -1; *l.choice = -1; }
    __syncthreads();
    float wpre = 0.f, total = 0.f;
#pragma unroll
    for (int w = 0; w < SAMP_NW; ++w) {
        if (w == (tid >> 6)) wpre = total;
        total += l.scan[w];
    }
    *total_out = total;
    return wpre + (inc - loc);
}
// the pre-draw probabilities, what the tests compare exactly
template <int MAXE> __device__ __forceinline__ void write_probs(const float (&e)[MAXE], float total, int V, int b, float* probs_out) {
    const int tid = threadIdx.x;
    const float inv = 1.0f / total;
#pragma unroll
    for (int j = 0; j < MAXE; ++j)
        if (tid + SAMP_NT * j < V) probs_out[(int64_t)b * V + tid + SAMP_NT * j] = e[j] * inv;
}
// ---- draw: u from Philox4x32-10 keyed by the seed, counter ctr = (stream, step, step >> 32, tag); inverse CDF over the kept set in
// thread-major order.  torch.multinomial's stream cannot be reproduced on device: equality with the reference is distributional, the
// pre-draw probabilities are compared exactly (probs_out).  Returns the id (0 for an empty distribution).
template <int MAXE> __device__ __forceinline__ int draw_id(const float (&e)[MAXE], float loc, float pre, float total, uint64_t seed, uint32_t (&ctr)[4], const
        SampleLds& l) {
    const int tid = threadIdx.x;
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), ctr);
    const float u = (float)(ctr[0] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
    const float target = u * total;
    if (loc > 0.f && pre <= target) atomicMax(l.thread, tid);  // thread 0's pre == 0 <= target
    __syncthreads();
    if (tid == *l.thread) {
        float acc = pre;
        int pick = -1, last = -1;
#pragma unroll
        for (int j = 0; j < MAXE; ++j) {
            if (e[j] > 0.f && pick < 0) {
                last = j;
                acc += e[j];
                if (acc > target) pick = j;
            }
        }
        const int jj = pick >= 0 ? pick : last;
        *l.choice = jj >= 0 ? tid + SAMP_NT * jj : -1;
    }
    __syncthreads();
    return *l.choice >= 0 ? *l.choice : 0;
}
// ---- commit.  GRAMMAR: the row's bookkeeping thread moves the row's state behind the id `id` the step commits: two dependent scalar
// loads and one plain store (one writer per row, read by the next step's kernel).  state < 0: the row has no grammar or was finished at
// step start, nothing is touched.  A banned id (only a forced one can be) leaves the state and sets bit 1 of the error flags.
__device__ __forceinline__ void grammar_advance_row(const GrammarArgs& gr, int b, int id, int state) {
    if (threadIdx.x != 0 || state < 0) return;
    const uint32_t c = (uint32_t)gr.class_of[id];
    const int ns = c < (uint32_t)gr.n_class ? gr.next[(int64_t)state * gr.n_class + c] : -1;
    if (ns >= 0) gr.state_out[b] = ns;
    else if (gr.err_flag) atomicOr(gr.err_flag, 2);
}
// the id goes to ids_out[b], or through the fused tail (which writes ids_out[b] too, does the row's loop bookkeeping and the NEXT
// step's embedding, and with PENALTY adds the id to the row's bitmap)
template <bool PENALTY, bool GRAMMAR, bool SCORED>
__device__ __forceinline__ void commit_id(int b, int id, const GrammarArgs& gr, int gstate, const TailArgs& tail, int fuse_tail, int32_t* ids_out, const
        RowLoop& st, float* sh_tail, uint32_t* presence) {
    if constexpr (GRAMMAR) grammar_advance_row(gr, b, id, gstate);
    if constexpr (SCORED) {
        if (!fuse_tail) __syncthreads();   // (the fused tail has barriers of its own before thread 0 reads the mass)
    }
    if (fuse_tail) advance_embed_row<PENALTY>(b, id, tail, ids_out, st.step, st.fed, st.len, st.done, st.stops, sh_tail, presence);
    else if (threadIdx.x == 0) ids_out[b] = id;
}
// SCORED (the instantiations with a ScoreArgs argument; common.h): the row also reports how likely its id was, and may be told its id.
//   * raw log-probability: raw_logsumexp's two words and x_id, re-read from the row here.
//   * choice log-probability: log(e_id / total) of the final distribution, -inf for an id outside the kept set (a forced one).
//   * forced id: >= 0 replaces the drawn id for everything downstream (>= V: clamped, bit 0 of the error flag).
// With a fused tail both values are filed at the row's step in the histories, after the next step's embedding is on its way; a row that
// was already finished files 0.  Without one they go to [B] vectors (advance_kernel files them).
template <int MAXE, bool PENALTY, bool GRAMMAR>
__device__ __forceinline__ void score_and_commit(const float (&e)[MAXE], float total, const float* lg, int V, int b, int tok, int forced, const ScoreArgs& sc,
        const GrammarArgs& gr, int gstate, const TailArgs& tail, int fuse_tail, int32_t* ids_out, const RowLoop& st, float* sh_tail, uint32_t* presence) {
    constexpr int NT = SAMP_NT; const int tid = threadIdx.x;
    int tk = tok;
    float x_id = 0.f;
    float* s_sc = score_lds();
    if (forced >= 0) {
        if (forced >= V) {
            forced = V - 1;
            if (tid == 0 && sc.err_flag) atomicOr(sc.err_flag, 1);
        }
        tk = forced;
    }
    if (tid == (tk & (NT - 1))) {   // the owner of logit tok has its mass in the final distribution (0: not kept)
        const int jj = tk / NT;
        float ev = 0.f;
#pragma unroll
        for (int j = 0; j < MAXE; ++j) ev = j == jj ? e[j] : ev;
        s_sc[2] = ev;
    }
    if (tid == 0) x_id = lg[tk];   // an L2 hit; in flight under the tail
    commit_id<PENALTY, GRAMMAR, true>(b, tk, gr, gstate, tail, fuse_tail, ids_out, st, sh_tail, presence);
    if (tid == 0) {
        float lp = x_id - s_sc[0] - s_sc[1];
        float ch = s_sc[2] > 0.f ? logf(s_sc[2] / total) : -INFINITY;
        int64_t at = b;
        bool file = true;
        if (fuse_tail) {
            if (st.done) lp = ch = 0.f;
            at = (int64_t)b * sc.out_stride + st.step;
            file = st.step < sc.out_stride;
        }
        if (file) {
            sc.logprob[at] = lp;
            if (sc.choice) sc.choice[at] = ch;
        }
    }
}
// One SAMP_NT-thread workgroup per row; thread t owns the logits t, t + SAMP_NT, ... in registers (MAXE of them).  (Round 4 measured
// two ways of spending more hardware on a row, both NEUTRAL: 1024 threads per row -- 21.9 / 32.3 us for top-k / top-p at B = 64, V = 8324
// against 20 / 31.9 -- and per-lane counters with one DPP reduction per pass instead of a ballot + s_bcnt1 per logit -- 22.8 us.  What did
// pay is taking the row out of the passes: "top-k without a pass over the row per bit" and "top-p without a top-k" above, 21.0 -> 11.5
// and 29.6 -> 20.5 us.)
// The optional parts are PENALTY, BIAS and the trailing pack (ScoreArgs, GrammarArgs, TruncArgs, at most one each, in this order): with
// the empty pack the argument list, and with every optional part under `if constexpr` the code, are the kernel's before that part.
// top_k == 1 is the argmax path (rowops.hip, ties to the lowest id) for the ids.  With records, or in the PENALTY / BIAS forms, a
// top_k == 1 row is the greedy step of a processed generation: the kept entry is the exact argmax of its processed row (lowest id
// among equals), so the temperature division -- which could merge neighbours -- is skipped.
template <int MAXE, bool PENALTY, bool BIAS, typename... Score>
__global__ __launch_bounds__(SAMP_NT) void sample_kernel(const float* __restrict__ logits, int V, SamplerParams pv,
                                                    const SamplerParams* __restrict__ pd, const int32_t* __restrict__ row_step,
                                                    int64_t step_host, int32_t* __restrict__ ids_out, float* __restrict__ probs_out,
                                                    TailArgs tail, int fuse_tail, int wave_select, uint32_t* __restrict__ presence,
                                                    const float* __restrict__ bias, Score... score) {
    constexpr bool SCORED = (std::is_same_v<Score, ScoreArgs> || ...);
    constexpr bool GRAMMAR = (std::is_same_v<Score, GrammarArgs> || ...);
    constexpr bool TRUNC = (std::is_same_v<Score, TruncArgs> || ...);
    static_assert(sizeof...(Score) == (SCORED ? 1 : 0) + (GRAMMAR ? 1 : 0) + (TRUNC ? 1 : 0),
                  "at most one ScoreArgs, then at most one GrammarArgs, then at most one TruncArgs");
    static_assert(!GRAMMAR || (PENALTY && BIAS), "the GRAMMAR form is built on the BIASED one");
    static_assert(!TRUNC || (PENALTY && BIAS), "the truncating form is built on the BIASED one");
    static_assert(MAXE <= 64, "the grammar's verdicts of a thread fit one 64-bit word");
    [[maybe_unused]] const ScoreArgs sc = extra_arg<ScoreArgs>(score...);
    [[maybe_unused]] const GrammarArgs gr = extra_arg<GrammarArgs>(score...);
    [[maybe_unused]] const TruncArgs ta = extra_arg<TruncArgs>(score...);
    constexpr int NT = SAMP_NT, NW = SAMP_NW;
    static_assert(SAMP_KFAST == 64 && NT == 256, "wave_publish_ge fills one slot per lane; the mass histogram has one bucket per thread");
    // ---- LDS.  Every instantiation: SampleLds says who owns what and what is reused ...
    __shared__ unsigned long long red64[2 * NW];
    __shared__ uint32_t s_cand[NW * SAMP_KFAST];
    __shared__ unsigned long long s_hist[NT];
    __shared__ int s_tie[NW], s_fit[NW];
    __shared__ float redf[NW], s_scan[NW], s_low[NW];
    __shared__ int s_thread, s_choice;
    const SampleLds l{red64, s_cand, s_hist, s_tie, s_fit, redf, s_low, s_scan, &s_thread, &s_choice};
    __shared__ float sh_tail[8];   // the fused tail's
    // ... and the feature-owned objects, each used by its stage alone (an instantiation without the feature does not have them)
    [[maybe_unused]] __shared__ uint32_t s_pres[MAXE * NT / 32];                  // PENALTY: the row's presence words
    [[maybe_unused]] __shared__ uint32_t s_gram_words[MGEA_GRAMMAR_MAX_WORDS];    // GRAMMAR: the state's row of the allow bitmask
    [[maybe_unused]] __shared__ float s_rawm[NW], s_raws[NW];                     // SCORED: the raw row's partials (next to score_lds())
    [[maybe_unused]] __shared__ int s_first;                                      // TRUNC: the floors' survivor
    const int b = blockIdx.x, tid = threadIdx.x;
    if (pd) pv = pd[b];   // the row's device-resident scalars win over the by-value copy
    [[maybe_unused]] int gstate = -1;
    if constexpr (GRAMMAR) gstate = grammar_row_state(gr, b);
    const float temperature = pv.temperature, top_p = pv.top_p;
    const int top_k = pv.top_k;
    const uint64_t seed = ((uint64_t)pv.seed_hi << 32) | pv.seed_lo;
    const float* lg = logits + (int64_t)b * V;
    RowLoop st{0, 0, 0, 0, RowStops{0, 0, 0}};
    if (fuse_tail && tid == 0) {
        st.step = tail.s.row_step[b]; st.fed = tail.s.cur_ids[b]; st.len = tail.s.ctx_len[b]; st.done = tail.s.done[b];
        st.stops = row_stops(tail.s, b);
    }
    [[maybe_unused]] int forced = -1;
    if constexpr (SCORED) forced = forced_id(sc, row_step, step_host, b);
    // load the row, bias and classes
    float x[MAXE];
    load_row<MAXE>(lg, V, x);
    [[maybe_unused]] float bz[BIAS ? MAXE : 1];
    [[maybe_unused]] const bool biased = BIAS && pv.bias_on != 0;
    if constexpr (BIAS) load_bias<MAXE>(bias + (int64_t)b * V, V, biased, bz);
    [[maybe_unused]] int gcls[GRAMMAR ? MAXE : 1];
    [[maybe_unused]] unsigned long long gban = 0ull;
    if constexpr (GRAMMAR) load_classes<MAXE>(gr, V, gstate, gcls, s_gram_words);
    // raw log-sum-exp
    if constexpr (SCORED) raw_logsumexp<MAXE>(x, s_rawm, s_raws);
    // penalty, and the grammar's verdicts under its barrier
    if constexpr (PENALTY) {
        stage_presence(presence, V, b, s_pres);
        if constexpr (GRAMMAR) {
            if (gstate >= 0) gban = grammar_verdicts<MAXE>(gr, gcls, s_gram_words);
        }
        apply_penalty<MAXE>(x, V, pv.penalty, s_pres);
    }
    // bias, grammar mask and EOS ban
    if constexpr (BIAS) {
        if (biased) add_bias<MAXE>(x, bz);
        if constexpr (GRAMMAR) {
            if (gstate >= 0) ban_classes<MAXE>(x, gban);
        }
        // min_new: no EOS before the row has produced that many ids (its step index, the Philox counter's word 1)
        const int eos = pv.eos_id;
        if (eos >= 0 && eos < V && pv.min_new > 0 && step_of(row_step, step_host, b) < pv.min_new) ban_id<MAXE>(x, eos);
    }
    // temperature and row maximum
    float mx = temper_and_max<MAXE>(x, temperature, temperature != 1.0f && !((PENALTY || BIAS || pd) && top_k == 1), redf);
    uint32_t key[MAXE], whi[MAXE], wlo[MAXE];
    make_keys<MAXE>(x, V, key, whi, wlo);
    // top-k, top-p, truncation: the kept set becomes {j : kept(key[j], keep_key)}
    uint32_t keep_key = 0u;  // keep everything
    uint32_t cand[NW] = {};  // wave-select path: this lane's share of the candidates (all waves hold the same list)
    bool cand_cover = false; // ... and they contain every entry >= keep_key (no ties beyond top_k)
    if (top_k > 0 && top_k < V) keep_key = topk_stage<MAXE>(key, whi, wlo, top_k, wave_select, l, cand, cand_cover);
    if (top_p > 0.f && top_p < 1.f) keep_key = topp_stage<MAXE>(x, key, whi, wlo, mx, top_p, keep_key, cand, cand_cover, wave_select, l);
    if constexpr (TRUNC) truncate_stage<MAXE>(x, key, whi, wlo, mx, keep_key, top_k, ta.rows[b], l, &s_first);
    // final distribution and exclusive scan
    float e[MAXE], total;
    const float loc = kept_distribution<MAXE>(x, key, keep_key, mx, e);
    const float pre = exclusive_scan(loc, l, &total);
    if (probs_out) write_probs<MAXE>(e, total, V, b, probs_out);
    if (!ids_out) return;
    // draw
    uint32_t ctr[4] = {pd ? pv.stream : (uint32_t)b, (uint32_t)step_of(row_step, step_host, b), (uint32_t)(step_host >> 32), 0x6d676561u};
    const int tok = draw_id<MAXE>(e, loc, pre, total, seed, ctr, l);
    // score and commit
    if constexpr (SCORED) score_and_commit<MAXE, PENALTY, GRAMMAR>(e, total, lg, V, b, tok, forced, sc, gr, gstate, tail, fuse_tail, ids_out, st, sh_tail, presence);
    else commit_id<PENALTY, GRAMMAR, false>(b, tok, gr, gstate, tail, fuse_tail, ids_out, st, sh_tail, presence);
}
// One launch site: MAXE by the vocabulary, the optional arguments forwarded in the kernel's order.
template <bool PENALTY, bool BIAS, typename... Extra> static int launch_form(const SampleCall& c, hipStream_t st, const Extra&... extra) {
    static_assert(SAMP_NT * 56 >= MGEA_SAMPLER_MAX_VOCAB, "the register-resident row must hold the largest vocabulary");
    const TailArgs t = c.tail ? *c.tail : TailArgs{};
    auto kern = c.V <= SAMP_NT * 36 ? sample_kernel<36, PENALTY, BIAS, Extra...> : sample_kernel<56, PENALTY, BIAS, Extra...>;
    hipLaunchKernelGGL(kern, dim3(c.B), dim3(SAMP_NT), 0, st, c.logits, c.V, c.params, c.params_dev, c.row_step_dev, c.step_host, c.ids_out,
                       c.probs_out, t, c.tail ? 1 : 0, tune(TUNE_SAMPLER_WAVE_SELECT), c.presence, c.bias, extra...);
    MGEA_CHECK_HIP(hipGetLastError());
    return MGEA_OK;
}
// the forms without a grammar or truncation exist for every <PENALTY, BIAS>
template <typename... Extra> static int launch_any(const SampleCall& c, hipStream_t st, const Extra&... extra) {
    if (c.bias) return c.presence ? launch_form<true, true>(c, st, extra...) : launch_form<false, true>(c, st, extra...);
    return c.presence ? launch_form<true, false>(c, st, extra...) : launch_form<false, false>(c, st, extra...);
}
int launch_sample(const SampleCall& c, hipStream_t st) {
    const TailArgs* tail = c.tail;
    const GrammarArgs& g = c.grammar;
    const bool scored = c.score.logprob != nullptr, gram = g.class_of != nullptr, trunc = c.trunc.rows != nullptr;
    MGEA_REQUIRE(c.params_dev || c.params.temperature > 0.f, MGEA_EINVAL, "sampler: temperature must be > 0");
    MGEA_REQUIRE(c.V > 0 && c.V <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "sampler: vocab %d exceeds the register-resident row (%d)", c.V,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(!tail || (c.ids_out && tail->C % 4 == 0 && tail->C <= 4096 && tail_qkv0_ok(*tail)), MGEA_EINVAL, "sampler: bad fused-tail arguments");
    MGEA_REQUIRE(!c.presence || c.params_dev || (std::isfinite(c.params.penalty) && c.params.penalty > 0.f), MGEA_EINVAL,
                 "sampler: the repetition penalty must be finite and > 0");
    MGEA_REQUIRE(!c.bias || c.params_dev, MGEA_EINVAL, "sampler: a bias needs the rows' device records");
    MGEA_REQUIRE(!(gram || trunc) || (c.bias && c.presence && c.params_dev), MGEA_EINVAL,
                 "sampler: the grammar and the truncating form need records, presence bitmaps and the bias buffer");
    MGEA_REQUIRE(!gram || (g.next && g.allow && g.state_in && g.n_state > 0 && g.n_class > 0 && g.n_class <= MGEA_GRAMMAR_MAX_CLASSES &&
                           g.words == grammar_words(g.n_class) && (!c.ids_out || g.state_out)),
                 MGEA_EINVAL, "sampler: bad grammar arguments");
    MGEA_REQUIRE(scored || !c.score.forced, MGEA_EINVAL, "sampler: forced ids need the scored form");
    MGEA_REQUIRE(!scored || c.ids_out, MGEA_EINVAL, "sampler: a scored launch draws ids");
    // the grammar and the truncating forms are built on <PENALTY, BIAS> alone
    if (trunc && gram) return scored ? launch_form<true, true>(c, st, c.score, g, c.trunc) : launch_form<true, true>(c, st, g, c.trunc);
    if (trunc) return scored ? launch_form<true, true>(c, st, c.score, c.trunc) : launch_form<true, true>(c, st, c.trunc);
    if (gram) return scored ? launch_form<true, true>(c, st, c.score, g) : launch_form<true, true>(c, st, g);
    return scored ? launch_any(c, st, c.score) : launch_any(c, st);
}

}  // namespace mgea
