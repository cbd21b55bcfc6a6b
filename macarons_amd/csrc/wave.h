// Wave64 and workgroup reductions, scans and the arg-max of the decision: the one statement of each idiom behind the project's rule for
// deterministic results (a fixed summation order, integer sums where the order is free, torch.max's ordering for the decision).
// Included by common.h.
//
// Seen and left hand-written on purpose (NOTES.md, "One header for wave and workgroup reductions"): the block-sum scan of
// smp_block_sums (glue.hip: doubles, its Hillis-Steele association is part of the sampler's bits); the arg-min of knn_grid_kernel
// (knn.hip: another rule, no NaN case); the __shfl(alpha, 4 * g + r) broadcasts of the attention kernels and every ballot; the
// local-transformer family.  Left hand-written as well, each with a comment at the site, because the call reschedules a hot kernel: the
// row reductions of attention_mfma_kernel and pool_long_kernel (nn_kernels.hip), the tile maximum of knn_mfma_kernel and the 8-lane
// query boxes of knn_grid_kernel (knn.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mcr {

// ---- wave64 DPP reductions ---------------------------------------------------------------------------
// After wave_sum_to_last(), lane 63 holds the sum of all 64 lanes (other lanes hold partial garbage).
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ float dpp_mov0(float v) {
    // old = 0, bound_ctrl = true: lanes without a source read 0.
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK,
                                                                 BANK_MASK, true));
}

__device__ __forceinline__ float wave_sum_to_last(float v) {
    v += dpp_mov0<0x111>(v);             // row_shr:1
    v += dpp_mov0<0x112>(v);             // row_shr:2
    v += dpp_mov0<0x114>(v);             // row_shr:4
    v += dpp_mov0<0x118>(v);             // row_shr:8   -> lane 15 of every row = row sum
    v += dpp_mov0<0x142, 0xa>(v);        // row_bcast:15 into rows 1,3
    v += dpp_mov0<0x143, 0xc>(v);        // row_bcast:31 into rows 2,3 -> lane 63 = wave sum
    return v;
}

// The two cross-row steps as ONE instruction each: `v_add_f32_dpp v, v, v row_bcast:15 row_mask:0xa` adds the broadcast lane in the
// enabled rows and leaves the other rows' v alone, which is what `v += dpp_mov0<0x142, 0xa>(v)` means -- but hipcc compiles
// that to v_mov 0 + v_mov_dpp + v_add (it only folds full-mask DPP moves).  Same additions in the same order as
// wave_sum_to_last().  The s_nop's are the two wait states a DPP read needs after a vector write of its source (the hazard
// recogniser does not look inside inline asm).
__device__ __forceinline__ float wave_sum_cross_rows(float v) {
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(v));
    return v;
}

// G independent reductions, step-major: the chains hide each other's DPP wait states.
template <int G>
__device__ __forceinline__ void wave_sum_to_last_multi(float (&v)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] += dpp_mov0<0x111>(v[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] += dpp_mov0<0x112>(v[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] += dpp_mov0<0x114>(v[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] += dpp_mov0<0x118>(v[g]);
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] = wave_sum_cross_rows(v[g]);
}

// ---- butterflies over the xor offsets ------------------------------------------------------------------
// The operators of a butterfly step, op(mine, the other lane's): fmaxf / fminf on floats (a NaN loses to a number), max / min on integers.
struct op_add {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct op_max {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); }
};
struct op_min {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); }
};

// v = op(v, v of lane ^ o) for the xor offsets o = FIRST, ..., LAST only, in THAT order (halving when FIRST > LAST, doubling
// otherwise): every lane of a group of lanes that differ in those bits ends with the group's result.  The order is part of a
// floating-point sum's bits, so a call site spells the one it always had: <16, 1> a half wave's 16 lanes, <16, 32> the four rows of
// a wave, <32, 32> its two halves, <1, 2> quads.
template <int FIRST, int LAST, typename T, typename Op>
__device__ __forceinline__ T lanes_reduce(T v, Op op) {
    if constexpr (FIRST > LAST) {
#pragma unroll
        for (int o = FIRST; o >= LAST; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    } else {
#pragma unroll
        for (int o = FIRST; o <= LAST; o <<= 1) v = op(v, __shfl_xor(v, o, 64));
    }
    return v;
}

// Every lane gets the sum of all 64 lanes, offsets 32 down to 1: the association of every full-wave sum here.
template <typename T>                                  // float, double, int, unsigned, long long
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Every lane gets the largest / smallest of all 64 lanes.
template <typename T>                                  // float, int, unsigned
__device__ __forceinline__ T wave_max_all(T v) { return lanes_reduce<32, 1>(v, op_max{}); }
template <typename T>
__device__ __forceinline__ T wave_min_all(T v) { return lanes_reduce<32, 1>(v, op_min{}); }

// Bounding box of N axes over every group of WIDTH consecutive lanes (offsets WIDTH / 2 down to 1): lo[a] <- min, hi[a] <- max, in
// every lane of the group.  Step-major like wave_sum_to_last_multi: the 2 N chains hide each other's latency.
template <int N, int WIDTH = 64>
__device__ __forceinline__ void wave_minmax(float (&lo)[N], float (&hi)[N]) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1)
#pragma unroll
        for (int a = 0; a < N; ++a) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
}

// The four wave totals of a 256-thread workgroup, `stride` apart, added in the one fixed association.
template <typename T>
__device__ __forceinline__ T four_wave_sum(const T* red, int stride = 1) {
    return (red[0] + red[stride]) + (red[2 * stride] + red[3 * stride]);
}

// Sum of v over the workgroup's 256 threads in a fixed order, through red[4] in LDS; every thread gets it after the barrier inside.
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T* red) {
    v = wave_sum_all(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return four_wave_sum(red);
}

// ---- scans -------------------------------------------------------------------------------------------
// Lane l gets v of lanes 0 .. l added up (Hillis-Steele over the wave: offsets 1 up to 32).  int, unsigned, double.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Exclusive scan of one integer per thread over a workgroup of NWAVES waves: the wave scan, the wave totals through s_wave[NWAVES] in
// LDS, then a serial base.  Returns the sum of v over the threads in front; *total (if asked for) gets the workgroup's sum, in
// every thread.  Integers only: the association is free.  EVERY thread of the workgroup must reach it (one barrier inside).
// SCRATCH_BUSY: s_wave may still be read by a previous call (a loop of rounds over one scratch) -- a barrier goes in front.
template <int NWAVES, bool SCRATCH_BUSY = false, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s_wave, T* total = nullptr) {
    static_assert(T(1) / 2 == 0, "integers only");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_inclusive_scan(v);
    if (SCRATCH_BUSY) __syncthreads();
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    T base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < NWAVES; ++k) {
        if (k < w) base += s_wave[k];
        all += s_wave[k];
    }
    if (total) *total = all;
    return base + inc - v;
}

// ---- the arg-max of the decision (testers/shapenet.py:172 = torch.max over the cameras) ------------------------------------
// torch.max's ordering, stated once: (v, i) comes before (bv, bi) when v is NaN and bv is not (NaN beats every number), else when v
// is the larger number, else -- equal values, or both NaN -- when i is the lower index (ties to the lower index, the first NaN
// wins).  Indices travel as fp32 (camera indices < 2^24 are exact).  The scorer's record, a single-rank decision and the merge of a
// sharded one all decide by this predicate.
__device__ __forceinline__ bool best_before(float v, float i, float bv, float bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;
}

// The 64-lane butterfly of that ordering: afterwards every lane holds the wave's best (value, index).
__device__ __forceinline__ void wave_best(float& bv, float& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64), oi = __shfl_xor(bi, o, 64);
        if (best_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

}  // namespace mcr
