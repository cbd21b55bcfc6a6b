// The SH scorer's per-point building blocks, shared by the forward (sh_scorer.hip) and the backward (sh_scorer_bwd.hip):
// the trig-free monomial form of z = sum_k Y_k(d) h_k, the coefficient transform and its transpose, and the tile load / store
// through the wave's LDS strip.
#pragma once
#include "common.h"
#include "sh_consts.inc"

namespace mcr {

__device__ __forceinline__ constexpr int shk(int l, int m) { return l * l + l + m; }

// z = sum_k Y_k(d) h_k, trig-free and in monomial form (algebra and constants: gen_sh_consts.py):
//   n = d / |d|  (one v_rsq);  x = cos(polar) = n_y;   sin(polar)^m {cos,sin}(m azim) = {Re,Im} (n_z + i n_x)^m
// so sin(polar), the azimuth normalisation 1/rho and the rho = 0 special case never appear (a ray along +-Y
// simply has n_x = n_z = 0 and every m != 0 term vanishes; the reference's acos path is ill-conditioned there).
// P_l^m / sin^m is a polynomial of degree l-m in x, so for one point the sum over l of each order m collapses into
// ONE polynomial per (m, cos|sin):  U_m(x) = sum_k a[m+k,+m] x^k,  V_m(x) = sum_k a[m+k,-m] x^k, whose coefficients
// a (64 per point, same storage as the SH coefficients) are produced once per point by to_mono_coeffs.  Then
//   z = U_0(x) + sum_{m>=1} ( Re w^m U_m(x) + Im w^m V_m(x) ),   w = n_z + i n_x
// and the sum over the orders is itself a Horner evaluation, in w over the complex numbers (below): 49 Horner FMAs in x
// + 24 for the six complex steps + 2 for the last real part + 7 to normalise = 82 VALU ops per (point, camera) pair (94 in the
// gain kernel's loop with the ray, the activation and the wave reduction).  The form this replaces kept the powers w^m
// (4 ops per order) and combined cm U_m + sm V_m into z (2 per order, a serial 14-step chain): 94 / 106 ops, gain kernel
// 50.4 -> 46.5 us at N = 100k, C = 200 (results 1.2e-7 apart); the rescaled-recurrence form before that needed 130.
// Measured on MI355X (tools/ubench): a dependent v_fma_f32 chain issues every ~8.8 cycles per wave; the 15 Horner
// chains are independent.  A packed form ((U_m, V_m) as ONE v_pk_fma_f32 chain per order: 70 instead of 106 vector
// instructions per pair) was built and measured (sh_dot_pk_rate.hip, NOTES): a packed instruction costs two scalar ones in
// this stream -- sh_dot alone 295 -> 275 cycles per pair and SIMD at 6 waves, the kernel 50.3 -> 50.0 us -- not kept.
// z = U_0(x) + Re( sum_{m>=1} w^m (U_m - i V_m) ): the sum over the orders as ONE complex Horner evaluation in w
//   A_7 = P_7,  A_m = A_{m+1} w + P_m  (m = 6..1),  z = U_0 + Re(w A_1),   P_m = U_m(x) - i V_m(x),  A = ar - i bi
// -- 4 FMAs per order instead of 4 for the power w^m and 2 to combine, and no serial 14-step accumulation into z.
__device__ __forceinline__ float sh_dot(float dx, float dy, float dz, const float (&a)[64]) {
    const float r2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float ir = __builtin_amdgcn_rsqf(r2);
    const float nx = dx * ir, ct = dy * ir, nz = dz * ir;
    float z = a[shk(7, 0)];
#pragma unroll
    for (int l = 6; l >= 0; --l) z = fmaf(ct, z, a[shk(l, 0)]);
    float ar = a[shk(7, 7)], bi = a[shk(7, -7)];
#pragma unroll
    for (int m = 6; m >= 1; --m) {
        float U = a[shk(7, m)], V = a[shk(7, -m)];
#pragma unroll
        for (int l = 6; l >= m; --l) {
            U = fmaf(ct, U, a[shk(l, m)]);
            V = fmaf(ct, V, a[shk(l, -m)]);
        }
        const float nr = fmaf(ar, nz, fmaf(bi, nx, U));
        const float nb = fmaf(bi, nz, fmaf(-ar, nx, V));
        ar = nr; bi = nb;
    }
    return fmaf(nz, ar, fmaf(nx, bi, z));
}

// One point's 64 SH coefficients -> VGPRs as the monomial coefficients of its 15 polynomials in cos(polar):
//   a[m+k, +-m] = sum_{l = m+k, m+k+2, ... < 8} SH_MONO[m][l][k] * h[l, +-m]      (in place: a[m+k] only needs h[l >= m+k])
// SCALE multiplies every coefficient (compile-time: folded into the SH_MONO immediates): the sigmoid kernels evaluate
// -log2(e) * z directly, the argument of their v_exp_f32.
template <bool SCALED = false>
__device__ __forceinline__ void to_mono_coeffs(float (&a)[64]) {
    constexpr float S = SCALED ? -1.4426950408889634f : 1.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int k = 0; k + m < 8; ++k) {
            float u = a[shk(m + k, m)] * (S * SH_MONO[m][m + k][k]);
            float v = a[shk(m + k, -m)] * (S * SH_MONO[m][m + k][k]);
#pragma unroll
            for (int l = m + k + 2; l < 8; l += 2) {
                u = fmaf(a[shk(l, m)], S * SH_MONO[m][l][k], u);
                v = fmaf(a[shk(l, -m)], S * SH_MONO[m][l][k], v);
            }
            a[shk(m + k, m)] = u;
            if (m) a[shk(m + k, -m)] = v;
        }
}

// The transpose of to_mono_coeffs<false>, for the backward: gradients with respect to the monomial coefficients
// (g[shk(m+k, +-m)] = dz/da) -> gradients with respect to the SH coefficients, in place:
//   dh[l, +-m] = sum_{k >= 0, m+k <= l, l-m-k even} SH_MONO[m][l][k] * g[m+k, +-m]
// (l descending: dh[l] reads only g[<= l], which are still untouched).
__device__ __forceinline__ void from_mono_grads(float (&g)[64]) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int l = 7; l >= m; --l) {
            float u = g[shk(l, m)] * SH_MONO[m][l][l - m];
            float v = g[shk(l, -m)] * SH_MONO[m][l][l - m];
#pragma unroll
            for (int k = l - m - 2; k >= 0; k -= 2) {
                u = fmaf(g[shk(m + k, m)], SH_MONO[m][l][k], u);
                v = fmaf(g[shk(m + k, -m)], SH_MONO[m][l][k], v);
            }
            g[shk(l, m)] = u;
            if (m) g[shk(l, -m)] = v;
        }
}

// The 64 x 64 coefficients of a wave-tile -> one row per lane.  A lane reading its own 256-byte row with sixteen 16-byte loads
// makes every load instruction of the wave touch 64 different cache lines (1024 line requests for 128 lines; the L1 of the CU,
// shared by 24 such waves, cannot hold them between instructions): the fixed part of a launch was 10 us of 53.  Here four
// neighbouring lanes read one 64-byte piece of a row (16 lines per instruction, each line in two instructions), the 16 loads are
// all in flight together, and the tile is turned by quarters through a 5 KB strip of LDS that only this wave touches (DS
// operations of one wave execute in order: no barrier; rows padded to 80 bytes).  Rows past the end of the cloud repeat its last row.
struct ScStage { float4 q[MCR_WAVE][5]; };
__device__ __forceinline__ void load_tile_rows(const float* __restrict__ harm_b, int row0, int N, int lane, ScStage& st,
                                               float (&a)[64]) {
    asm volatile("" : "+v"(lane));      // addresses derived from the lane index are rebuilt per tile, not kept live through the camera loop
    const int chunk = lane & 3, rsub = lane >> 2;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 v[4][4];                                             // [column quarter][row group]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // uniform base + 32-bit byte offset (the scalar-base addressing form: one address register per row group)
        const float* src = reinterpret_cast<const float*>(reinterpret_cast<const char*>(harm_b) +
                                                          (unsigned)(min(row0 + 16 * i + rsub, N - 1) * 256 + 16 * chunk));
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p][i] = *reinterpret_cast<const f32x4*>(src + 16 * p);
    }
    // In place: the four row groups of a quarter go out and the lane's own row comes back into the SAME registers (written as
    // one asm block with tied operands; left to the register allocator the turn needed 101 VGPRs and cost two resident waves).
    const unsigned wa = (unsigned)(size_t)&st.q[rsub][chunk], ra = (unsigned)(size_t)&st.q[lane][0];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        asm volatile("ds_write_b128 %4, %0\n\t"
                     "ds_write_b128 %4, %1 offset:%c6\n\t"
                     "ds_write_b128 %4, %2 offset:%c7\n\t"
                     "ds_write_b128 %4, %3 offset:%c8\n\t"
                     "ds_read_b128 %0, %5\n\t"
                     "ds_read_b128 %1, %5 offset:16\n\t"
                     "ds_read_b128 %2, %5 offset:32\n\t"
                     "ds_read_b128 %3, %5 offset:48\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "+v"(v[p][0]), "+v"(v[p][1]), "+v"(v[p][2]), "+v"(v[p][3])
                     : "v"(wa), "v"(ra), "n"(16 * 80), "n"(32 * 80), "n"(48 * 80)
                     : "memory");
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[16 * p + 4 * c + 0] = v[p][c].x; a[16 * p + 4 * c + 1] = v[p][c].y;
            a[16 * p + 4 * c + 2] = v[p][c].z; a[16 * p + 4 * c + 3] = v[p][c].w;
        }
    }
    // plain 32-bit values from here on: with the coefficients still tied to their 128-bit tuples the instruction scheduler
    // orders the camera loop differently (same instructions), 7 % slower per camera
#pragma unroll
    for (int k = 0; k < 64; ++k) asm volatile("" : "+v"(a[k]));
}

// The inverse of load_tile_rows: one 256-byte row per lane -> rows row0.. of out_b, through the same LDS strip by quarters.  A lane
// drops a quarter of its row into the strip, then four neighbouring lanes store one 64-byte piece of a row (16 rows per store
// instruction, not 64 lines).  DS operations of one wave execute in order; the wave barriers only keep the compiler from moving the
// strip's writes and reads across each other.  Rows at or past N are not written.
__device__ __forceinline__ void store_tile_rows(float* __restrict__ out_b, int row0, int N, int lane, ScStage& st,
                                                const float (&a)[64]) {
    const int chunk = lane & 3, rsub = lane >> 2;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            st.q[lane][c] = make_float4(a[16 * p + 4 * c + 0], a[16 * p + 4 * c + 1], a[16 * p + 4 * c + 2], a[16 * p + 4 * c + 3]);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 16 * i + rsub;
            const float4 v = st.q[16 * i + rsub][chunk];
            if (row < N) *reinterpret_cast<float4*>(out_b + (size_t)row * 64 + 16 * p + 4 * chunk) = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace mcr
