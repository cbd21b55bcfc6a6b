// K9 — spherical-harmonic coverage-gain scorer for gfx950 (MI355X).
//
// Replaces the op sequence of the reference's
//   macarons/networks/SconeVis.py:210-252  compute_coverage_gain   -> gains [B,C]
//   macarons/networks/SconeVis.py:164-208  compute_visibilities    -> vis   [B,C,N]
//   (== macarons/networks/Macarons.py:138-178 compute_visibility_gains)
// which materialise [B*C*N,64] SH tensors three times.  Here: one lane owns one point (its 64 SH
// coefficients live in VGPRs, turned once into the monomial coefficients of 15 polynomials in cos(polar)), cameras
// come from wave-uniform scalar loads, the dot with the 64 real SH of the ray direction is evaluated trig-free by
// Horner steps (82 VALU ops per (point,camera) pair, 94 with activation and reduction), sigmoid/relu applied, and the per-camera sum over points
// is a wave64 DPP reduction -> per-wave-tile partials -> a deterministic second-pass reduce (bit-stable
// run to run).  Bound: fp32 VALU (370 algorithmic flop / pair; N*268 B of HBM per cloud).
//
// Conventions (reference CustomGeometry.py:27-45, spherical_harmonics.py:67-140): polar axis +Y,
// azimuth from +Z toward +X; channel k = l*l + l + m; Condon-Shortley phase included.
#include "sh_mono.h"
#include <algorithm>

namespace mcr {

constexpr int SC_BLOCK = 256;       // 4 waves; one point per lane

// Workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8) and every XCD has its own L2.  Consecutive wave ranges
// share a wave-tile's coefficients at their boundary, so the ranges are handed out in XCD-major order: the blocks of one
// XCD own one contiguous stretch of the unit space and a tile cut by a block boundary is fetched into one L2 only
// (measured HBM reads per launch: 68.6 MB with the plain order, 27.6 MB with this one; algorithmic 26.8 MB).
__device__ __forceinline__ int xcd_major_block(int b, int nb) {
    const int x = b & 7, q = nb >> 3, r = nb & 7;            // XCD x holds q + (x < r) blocks
    return x * q + (x < r ? x : r) + (b >> 3);
}

// SIGMOID: zs = -log2(e) * z (the coefficients carry the factor, to_mono_coeffs<true>): 1 / (1 + exp(-z)) = 1 / (1 + 2^zs).
template <bool SIGMOID>
__device__ __forceinline__ float activate(float zs) {
    if (SIGMOID) return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(zs));
    return fmaxf(zs, 0.f);
}

// Lanes past the end of the cloud (last wave-tile only) carry the cloud's last point with the constant coefficient replaced by
// -1e30 (scaled form: +1e30), so z = -1e30 and the activation is exactly 0 (sigmoid: 2^(+1e30) = inf, 1 / inf = 0; relu:
// max(z, 0) = 0) -- no per-pair masking multiply.
template <bool SIGMOID>
__device__ __forceinline__ void blank_lane(bool valid, float (&a)[64]) {
    float big;
    asm volatile("v_mov_b32 %0, %1" : "=v"(big) : "n"(SIGMOID ? 0x7149f2ca : 0xf149f2ca));     // +-1e30, made here (not kept live through the camera loop)
    a[0] = valid ? a[0] : big;
}

// ---- work decomposition (both kernels) ----------------------------------------------------------------------
// A "wave-unit" is (wave-tile of 64 points, camera).  The U = B * ceil(N/64) * C units are split into W equal
// contiguous ranges, one per wave, with W = min(U, co-resident waves of the chip): the whole grid is resident
// and every wave finishes at the same time (measured: equal-size blocks needing 2.14 rounds cost 3).  A wave
// walks its range as segments (one wave-tile x a camera range): it loads the tile's 64x64 coefficients into
// VGPRs once per segment, then loops over the cameras (wave-uniform -> scalar loads).  No LDS, no barriers.
//
// ---- coverage-gain kernel (mean over points) ---------------------------------------------------------------
// The wave reductions of SC_R consecutive cameras can be issued together (step-major, hiding each other's DPP wait states) while
// the dot products still run one camera at a time.  Measured (100k points x 200 cameras, us per step): 58.6 / 62.0 / 65.2 / 65.3
// for SC_R = 1 / 2 / 3 / 4 -- the extra live values cost a resident wave per SIMD (80 VGPRs -> 6 waves at SC_R = 1, 90 -> 5 at 4),
// which outweighs the shorter tail; interleaving the dot products themselves (SC_G, round 1) lost the same way.  Each
// partial[b][c][wave-tile] is written by exactly one wave; the second pass adds them in a fixed order -> bit-stable results (no
// float atomics).
#ifndef SC_R_N
#define SC_R_N 1
#endif
constexpr int SC_R = SC_R_N;

template <bool SIGMOID>
__global__ __launch_bounds__(SC_BLOCK) void sh_gain_kernel(const float* __restrict__ pts, int pts_stride,
                                                           const float* __restrict__ harm,
                                                           const float* __restrict__ cams, float* __restrict__ partial,
                                                           int N, int C, int n_wtiles, long long U, int W) {
    __shared__ ScStage s_stage[SC_BLOCK / MCR_WAVE];
    const int lane = threadIdx.x & (MCR_WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(xcd_major_block(blockIdx.x, gridDim.x) * (SC_BLOCK / MCR_WAVE) + threadIdx.x / MCR_WAVE);
    if (w >= W) return;
    // The wave's range of units -> (cloud b, wave-tile wt, first camera, units left): divided ONCE, then walked (the quotients of a
    // per-segment division, and the reciprocal seeds of its expansion, stayed in vector registers through the camera loop).
    int b, wt, c_begin, left;
    {
        const long long u = (U * w) / W, bt = u / C;
        b = __builtin_amdgcn_readfirstlane((int)(bt / n_wtiles));
        wt = __builtin_amdgcn_readfirstlane((int)(bt - (long long)(bt / n_wtiles) * n_wtiles));
        c_begin = __builtin_amdgcn_readfirstlane((int)(u - bt * C));
        left = __builtin_amdgcn_readfirstlane((int)((U * (w + 1)) / W - u));
    }
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / MCR_WAVE);
    for (; left > 0; c_begin = 0, b += (wt + 1 == n_wtiles), wt = (wt + 1 == n_wtiles ? 0 : wt + 1)) {
        const int c_end = min(C, c_begin + left);
        left -= c_end - c_begin;
        const int n = wt * MCR_WAVE + lane;
        const bool valid = n < N;
        const size_t pn = (size_t)b * N + (valid ? n : N - 1);
        float hs[64];
        load_tile_rows(harm + (size_t)b * N * 64, wt * MCR_WAVE, N, lane, s_stage[wave_in_block], hs);
        const float px = pts[pn * pts_stride + 0];            // after the tile: its 64 landing registers are the peak
        const float py = pts[pn * pts_stride + 1];
        const float pz = pts[pn * pts_stride + 2];
        to_mono_coeffs<SIGMOID>(hs);
        blank_lane<SIGMOID>(valid, hs);
        const float* cam_b = cams + (size_t)b * C * 3;
        float* part_col = partial + (size_t)b * C * n_wtiles + wt;   // partial[b][:][wt]  (camera-major: the reduce reads rows)
        // Cameras are walked SC_R at a time: the SC_R dot products run one after the other (one camera's registers), the SC_R
        // wave reductions run together -- one reduction alone is six DEPENDENT DPP steps with nothing beside them (step-major
        // interleaving hides the wait states).  The camera centres are wave-uniform scalar loads; the next group's are requested
        // before this group's arithmetic (left in place, each iteration opens with an exposed scalar-cache round trip).
        float cn[SC_R][3];
#pragma unroll
        for (int c = 0; c < SC_R; ++c) {
            const int i = min(c_begin + c, c_end - 1);
            cn[c][0] = cam_b[3 * i + 0]; cn[c][1] = cam_b[3 * i + 1]; cn[c][2] = cam_b[3 * i + 2];
        }
        for (int ci = c_begin; ci < c_end; ci += SC_R) {
            float cc[SC_R][3];
#pragma unroll
            for (int c = 0; c < SC_R; ++c) {
                cc[c][0] = cn[c][0]; cc[c][1] = cn[c][1]; cc[c][2] = cn[c][2];
                const int i = min(ci + SC_R + c, c_end - 1);       // ragged tail: surplus slots repeat the last camera
                cn[c][0] = cam_b[3 * i + 0]; cn[c][1] = cam_b[3 * i + 1]; cn[c][2] = cam_b[3 * i + 2];
            }
            float sum[SC_R];
#pragma unroll
            for (int c = 0; c < SC_R; ++c) {
                // rays = X_cam - X_pts (SconeVis.py:230-231)
                const float z = sh_dot(cc[c][0] - px, cc[c][1] - py, cc[c][2] - pz, hs);
                sum[c] = activate<SIGMOID>(z);
                asm volatile("" : "+v"(sum[c]));             // one camera at a time: interleaving the dots costs a resident wave
            }
            wave_sum_to_last_multi<SC_R>(sum);
            if (lane == MCR_WAVE - 1) {
#pragma unroll
                for (int c = 0; c < SC_R; ++c)
                    if (ci + c < c_end) part_col[(size_t)(ci + c) * n_wtiles] = sum[c];
            }
        }
    }
}

// gains[b][c] = (sum_wt partial[b][c][wt]) / N ; one 256-thread block per (b,c) reading its contiguous row, fixed tree order.
__global__ __launch_bounds__(256) void sh_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gains,
                                                        int n_wtiles, int C, float inv_n) {
    __shared__ double s_w[4];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* p = partial + ((size_t)b * C + c) * n_wtiles;
    double acc = 0.0;
    for (int t = threadIdx.x; t < n_wtiles; t += 256) acc += (double)p[t];
    acc = wave_sum_all(acc);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) gains[(size_t)b * C + c] = (float)four_wave_sum(s_w) * inv_n;
}

// The decision behind the gains (testers/shapenet.py:172: torch.max over the cameras): record[b] = (max_c gains[b][c], first arg-max as
// fp32) with torch.max's ordering (best_before / wave_best of wave.h, shared with the decision glue).  One block per cloud.
__global__ __launch_bounds__(256) void sh_best_kernel(const float* __restrict__ gains, int C, float* __restrict__ record) {
    __shared__ float s_v[4], s_i[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    float bv = -__builtin_inff(), bi = 3.0e38f;
    bool first = true;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float g = gains[(size_t)b * C + c];
        if (first || best_before(g, (float)c, bv, bi)) { bv = g; bi = (float)c; }
        first = false;
    }
    wave_best(bv, bi);
    if (lane == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (best_before(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
        record[2 * b] = bv;
        record[2 * b + 1] = bi;
    }
}

// ---- per-point kernel (visibilities [B,C,N]) ---------------------------------------------------------------
template <bool SIGMOID>
__global__ __launch_bounds__(SC_BLOCK) void sh_vis_kernel(const float* __restrict__ pts, int pts_stride,
                                                          const float* __restrict__ harm,
                                                          const float* __restrict__ cams, float* __restrict__ out,
                                                          int N, int C, int n_wtiles, long long U, int W) {
    __shared__ ScStage s_stage[SC_BLOCK / MCR_WAVE];
    const int lane = threadIdx.x & (MCR_WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(xcd_major_block(blockIdx.x, gridDim.x) * (SC_BLOCK / MCR_WAVE) + threadIdx.x / MCR_WAVE);
    if (w >= W) return;
    // The wave's range of units -> (cloud b, wave-tile wt, first camera, units left): divided ONCE, then walked (the quotients of a
    // per-segment division, and the reciprocal seeds of its expansion, stayed in vector registers through the camera loop).
    int b, wt, c_begin, left;
    {
        const long long u = (U * w) / W, bt = u / C;
        b = __builtin_amdgcn_readfirstlane((int)(bt / n_wtiles));
        wt = __builtin_amdgcn_readfirstlane((int)(bt - (long long)(bt / n_wtiles) * n_wtiles));
        c_begin = __builtin_amdgcn_readfirstlane((int)(u - bt * C));
        left = __builtin_amdgcn_readfirstlane((int)((U * (w + 1)) / W - u));
    }
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / MCR_WAVE);
    for (; left > 0; c_begin = 0, b += (wt + 1 == n_wtiles), wt = (wt + 1 == n_wtiles ? 0 : wt + 1)) {
        const int c_end = min(C, c_begin + left);
        left -= c_end - c_begin;
        const int n = wt * MCR_WAVE + lane;
        const bool valid = n < N;
        const size_t pn = (size_t)b * N + (valid ? n : N - 1);
        float hs[64];
        load_tile_rows(harm + (size_t)b * N * 64, wt * MCR_WAVE, N, lane, s_stage[wave_in_block], hs);
        const float px = pts[pn * pts_stride + 0];
        const float py = pts[pn * pts_stride + 1];
        const float pz = pts[pn * pts_stride + 2];
        to_mono_coeffs<SIGMOID>(hs);
        const float* cam_b = cams + (size_t)b * C * 3;
        for (int ci = c_begin; ci < c_end; ++ci) {
            const float z = sh_dot(cam_b[3 * ci + 0] - px, cam_b[3 * ci + 1] - py, cam_b[3 * ci + 2] - pz, hs);
            const float v = activate<SIGMOID>(z);
            if (valid) out[((size_t)b * C + ci) * N + n] = v;
        }
    }
}

// Waves that are co-resident on the chip for `kernel` (occupancy API: from its real VGPR allocation).
template <typename Kern>
static int resident_waves(Kern kernel, int waves_per_simd_override) {
    int dev = 0, n_cu = 256, blocks_per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    if (waves_per_simd_override > 0) return n_cu * 4 * waves_per_simd_override;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, SC_BLOCK, 0) != hipSuccess || blocks_per_cu <= 0)
        blocks_per_cu = 4;
    return n_cu * blocks_per_cu * (SC_BLOCK / MCR_WAVE);
}

template <typename Kern>
static int resident_waves_cached(Kern kernel, int waves_per_simd_override, int* cache) {
    if (waves_per_simd_override > 0) return resident_waves(kernel, waves_per_simd_override);
    if (!*cache) *cache = resident_waves(kernel, 0);
    return *cache;
}

}  // namespace mcr

using namespace mcr;

extern "C" {

size_t mcr_sh_coverage_gain_workspace_bytes(int64_t B, int64_t N, int64_t C) {
    return (size_t)B * (size_t)cdiv(N, MCR_WAVE) * (size_t)C * sizeof(float);
}

static int sh_gain_impl(const char* who, bool reduce, const float* pts, int pts_dim, const float* harmonics, const float* cams,
                        float* gains, int64_t B, int64_t N, int64_t C, int use_sigmoid, int waves_per_simd, void* workspace,
                        size_t workspace_bytes, void* stream) {
    MCR_REQUIRE(pts && harmonics && cams && (gains || !reduce), "%s: null pointer", who);
    MCR_REQUIRE(pts_dim >= 3, "%s: pts_dim must be >= 3 (got %d)", who, pts_dim);
    MCR_REQUIRE(B > 0 && N > 0 && C > 0, "%s: empty problem B=%ld N=%ld C=%ld", who, (long)B, (long)N, (long)C);
    // N <= 2^23: load_tile_rows addresses a coefficient row as a 32-bit byte offset (row * 256) from the cloud's base
    MCR_REQUIRE(C <= 65535 * 64 && N <= (1ll << 23) && B <= 65535, "%s: problem too large (N <= 2^23 points per cloud)", who);
    MCR_REQUIRE(waves_per_simd >= 0 && waves_per_simd <= 16, "%s: waves_per_simd out of range", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_sh_coverage_gain_workspace_bytes(B, N, C), "%s: workspace too small", who);
    static int cache_sig = 0, cache_relu = 0;
    const int resident = use_sigmoid ? resident_waves_cached(sh_gain_kernel<true>, waves_per_simd, &cache_sig)
                                     : resident_waves_cached(sh_gain_kernel<false>, waves_per_simd, &cache_relu);
    const int n_wtiles = (int)cdiv(N, MCR_WAVE);
    const long long U = (long long)B * n_wtiles * C;
    const int W = (int)std::min<long long>(U, resident);
    MCR_REQUIRE(U / W < (1ll << 30), "%s: problem too large", who);          // a wave's unit count is an int
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)cdiv(W, SC_BLOCK / MCR_WAVE));
    float* partial = (float*)workspace;
    if (use_sigmoid)
        hipLaunchKernelGGL(sh_gain_kernel<true>, grid, dim3(SC_BLOCK), 0, s, pts, pts_dim, harmonics, cams, partial,
                           (int)N, (int)C, n_wtiles, U, W);
    else
        hipLaunchKernelGGL(sh_gain_kernel<false>, grid, dim3(SC_BLOCK), 0, s, pts, pts_dim, harmonics, cams, partial,
                           (int)N, (int)C, n_wtiles, U, W);
    MCR_LAUNCH_CHECK("sh_gain_kernel");
    if (!reduce) return 0;
    hipLaunchKernelGGL(sh_reduce_kernel, dim3((unsigned)C, (unsigned)B), dim3(256), 0, s, partial, gains, n_wtiles, (int)C,
                       1.0f / (float)N);
    MCR_LAUNCH_CHECK("sh_reduce_kernel");
    return 0;
}

int mcr_sh_coverage_gain(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* gains,
                         int64_t B, int64_t N, int64_t C, int use_sigmoid, int waves_per_simd, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return sh_gain_impl("mcr_sh_coverage_gain", true, pts, pts_dim, harmonics, cams, gains, B, N, C, use_sigmoid, waves_per_simd,
                        workspace, workspace_bytes, stream);
}

int mcr_sh_coverage_gain_best(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* gains, float* record,
                              int64_t B, int64_t N, int64_t C, int use_sigmoid, int waves_per_simd, void* workspace,
                              size_t workspace_bytes, void* stream) {
    MCR_REQUIRE(record, "mcr_sh_coverage_gain_best: null pointer");
    MCR_REQUIRE(C < (1ll << 24), "mcr_sh_coverage_gain_best: camera indices must stay below 2^24");
    if (int e = sh_gain_impl("mcr_sh_coverage_gain_best", true, pts, pts_dim, harmonics, cams, gains, B, N, C, use_sigmoid, waves_per_simd,
                             workspace, workspace_bytes, stream))
        return e;
    hipLaunchKernelGGL(sh_best_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, gains, (int)C, record);
    MCR_LAUNCH_CHECK("sh_best_kernel");
    return 0;
}

int mcr_sh_coverage_gain_partials(const float* pts, int pts_dim, const float* harmonics, const float* cams, int64_t B, int64_t N,
                                  int64_t C, int use_sigmoid, int waves_per_simd, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return sh_gain_impl("mcr_sh_coverage_gain_partials", false, pts, pts_dim, harmonics, cams, nullptr, B, N, C, use_sigmoid,
                        waves_per_simd, workspace, workspace_bytes, stream);
}

int mcr_sh_visibilities(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* vis,
                        int64_t B, int64_t N, int64_t C, int use_sigmoid, void* stream) {
    MCR_REQUIRE(pts && harmonics && cams && vis, "mcr_sh_visibilities: null pointer");
    MCR_REQUIRE(pts_dim >= 3, "mcr_sh_visibilities: pts_dim must be >= 3 (got %d)", pts_dim);
    MCR_REQUIRE(B > 0 && N > 0 && C > 0, "mcr_sh_visibilities: empty problem");
    MCR_REQUIRE(C < (1 << 24) && N <= (1ll << 23), "mcr_sh_visibilities: problem too large (N <= 2^23 points per cloud)");
    static int cache_sig = 0, cache_relu = 0;
    const int resident = use_sigmoid ? resident_waves_cached(sh_vis_kernel<true>, 0, &cache_sig)
                                     : resident_waves_cached(sh_vis_kernel<false>, 0, &cache_relu);
    const int n_wtiles = (int)cdiv(N, MCR_WAVE);
    const long long U = (long long)B * n_wtiles * C;
    const int W = (int)std::min<long long>(U, resident);
    MCR_REQUIRE(U / W < (1ll << 30), "mcr_sh_visibilities: problem too large");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)cdiv(W, SC_BLOCK / MCR_WAVE));
    if (use_sigmoid)
        hipLaunchKernelGGL(sh_vis_kernel<true>, grid, dim3(SC_BLOCK), 0, s, pts, pts_dim, harmonics, cams, vis, (int)N,
                           (int)C, n_wtiles, U, W);
    else
        hipLaunchKernelGGL(sh_vis_kernel<false>, grid, dim3(SC_BLOCK), 0, s, pts, pts_dim, harmonics, cams, vis, (int)N,
                           (int)C, n_wtiles, U, W);
    MCR_LAUNCH_CHECK("sh_vis_kernel");
    return 0;
}

}  // extern "C"
