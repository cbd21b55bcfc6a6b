// Register-tile helpers shared by the fused local transformers that keep the residual stream in registers (local_pct6.hip:
// fp16 hi/lo planes; local_pct7.hip: one fp16 plane), pulled into their namespaces with `using namespace tile`; local_pct5.hip
// takes opaque and rows_allreduce from here.  What differs per variant -- the weight ring, the product pipelines, the LDS
// addressing, the plane stores, LayerNorm, GELU, attention -- stays in the variant's own file.  So do the kernel bodies' short
// common blocks (xyz load and concatenation, the 2^-e scaling of the residual registers, soft-max, pooling): as functions they
// compile to different register assignments (NOTES.md, "Fused local transformers: shared tile helpers").
// Tile convention: a workgroup = 4 waves = 64 tokens (4 sequences x 16); a C fragment t (n-tile nt, m-tile mt) holds, in lane
// (j, h) = (lane & 31, lane >> 5), the features 32 nt + 8 g + 4 h + e (register r = 4 g + e) of token 32 mt + j.
#pragma once
#include "lp_split.h"

namespace mcr {
namespace tile {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The swizzled addresses are loop-invariant functions of the lane; left alone, LLVM hoists all of them out of the encoder
// loop and spills them (172 scratch stores in variant 5).  Re-deriving them from an opaque copy of the lane id per phase is
// cheaper.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Pin accumulator chains to this point of the program: the MFMA builtins are pure, so instruction selection is free to delay a
// whole chain to its next use (it deferred one m-tile's 24 MFMAs of a product past the following product and two barriers,
// spilling the fragments it had loaded for them).  An empty asm that "rewrites" the accumulators orders them like a fence.
__device__ __forceinline__ void pin(f32x16& a, f32x16& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void pin(f32x16& a, f32x16& b, f32x16& c) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c)); }

__device__ __forceinline__ void zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// The accumulator of a product starts from its bias: the four 16-byte loads land directly in the accumulator registers.
__device__ __forceinline__ void init_bias(f32x16& a, const float* __restrict__ vec, int nt, int lane_) {
    const float4* p = reinterpret_cast<const float4*>(vec + 32 * nt + 4 * (opaque(lane_) >> 5));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 b = p[2 * g];
        a[4 * g] = b.x; a[4 * g + 1] = b.y; a[4 * g + 2] = b.z; a[4 * g + 3] = b.w;
    }
}

// lanes l and l ^ 32 (the two halves of a token's 32 features in this wave): sum on both
__device__ __forceinline__ float halves_sum(float v) {
    const unsigned c = __builtin_bit_cast(unsigned, v);
    const auto q = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return __builtin_bit_cast(float, (unsigned)q[0]) + __builtin_bit_cast(float, (unsigned)q[1]);
}
// All-reduce over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48) without the LDS crossbar: gfx950's
// v_permlane16_swap / v_permlane32_swap exchange rows / halves between two registers; fed the same value twice they return
// (this row pair's even row | odd row) resp. (lower half | upper half) replicated, so one op on the pair is the reduction.
template <class Op>
__device__ __forceinline__ float rows_allreduce(float v, Op op) {
    const unsigned b = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    v = op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
    const unsigned c = __builtin_bit_cast(unsigned, v);
    const auto q = __builtin_amdgcn_permlane32_swap(c, c, false, false);
    return op(__builtin_bit_cast(float, (unsigned)q[0]), __builtin_bit_cast(float, (unsigned)q[1]));
}

// dev only: per-phase timestamps of one workgroup (tools/build_variant.py ... -DL6_TRACE=<block> or -DL7_TRACE=<block>, read
// by tools/trace_local_pct.py).  The kernel's file maps its own switch to LP_TRACE in front of this header; LP_T() needs the
// kernel's `tid` and a stamp counter `int tp = 0` in scope.
#ifdef LP_TRACE
__device__ long long lp_trace_buf[64];
#define LP_T() do { if (blockIdx.x == (LP_TRACE) && tid == 0) { lp_trace_buf[tp] = clock64(); lp_trace_buf[tp ? 63 : 62] = wall_clock64(); } ++tp; } while (0)
#else
#define LP_T() do { } while (0)
#endif

}  // namespace tile
}  // namespace mcr

#ifdef LP_TRACE
extern "C" int mcr_dev_read_trace(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mcr::tile::lp_trace_buf), sizeof(long long) * 64); }
#endif
