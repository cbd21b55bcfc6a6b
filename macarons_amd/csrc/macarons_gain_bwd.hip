// Backward of the MACARONS-regime coverage gain (macarons_gain_kernel, glue.hip; macarons_gain_inv_kernel, scene.hip) for gfx950: the
// last link of the chain upstream's online trainer differentiates (train_macarons.py:438-444 -> :507 / :753 -> :1259 through
// predict_coverage_gain_for_single_camera, macarons_utils.py:1580-1738).  With f the distance factor and
//   gains[k] = n_unique[k] > 0 ? volume[k] / S * sum_s vis_u[k, inv[k,s]] * f(|world_u[k, inv[k,s]] - cam_world[k]|) : 0
// an incoming g[k] gives
//   d_vis_u[k,u] = (g[k] * volume[k] / S) * count[k,u] * f(k,u),   count[k,u] = #{s : inv[k,s] == u}   (0 for u >= n_unique[k], and
//                  for every row of a camera with n_unique[k] == 0),
//   d_volume[k]  = g[k] * (the forward's mean of camera k)                                             (0 for n_unique[k] == 0).
// One workgroup per camera.  count is an int histogram in LDS built with integer LDS atomics -- order-independent, so the result is
// bit-reproducible; no floating-point atomic, no global atomic.  Then one thread per u writes d_vis_u.  The mean of d_volume is
// accumulated exactly as the forward accumulates it (double, the same sample order, the same lane / wave reduction order).
// MCR_HIPCC_FLAGS: -ffp-contract=off
#include "common.h"

namespace mcr {

constexpr int MGB_MAX_S = 8192;                      // counters in static LDS: 32 KB

// The distance factor of macarons_gain_kernel (glue.hip) and macarons_gain_inv_kernel (scene.hip), restated: the same operations in the
// same order (this file is compiled without FMA contraction, as those two are), so the bits are theirs.  mode 0 = min(1, (th / d)^2),
// mode 1 = 1 / (1 + (d / th)^2).
__device__ __forceinline__ float gain_distance_factor(const float* __restrict__ p, float cx, float cy, float cz, float distance_th, int mode) {
    const float dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    float f = 1.f;
    if (mode == 1) {
        const float q = d / distance_th;
        f = 1.f / (1.f + q * q);
    } else if (d > distance_th) {
        f = (distance_th * distance_th) / (d * d);
    }
    return f;
}

// inv == nullptr (then nu == nullptr too): the identity map, every camera non-empty -- the backward of macarons_gain_kernel.
__global__ __launch_bounds__(256) void macarons_gain_bwd_kernel(const float* __restrict__ g, const float* __restrict__ vis,
                                                                const float* __restrict__ world, int pts_dim,
                                                                const long long* __restrict__ inv, const int* __restrict__ nu,
                                                                const float* __restrict__ cam_world, const float* __restrict__ volume,
                                                                float distance_th, int mode, int S, float* __restrict__ d_vis,
                                                                float* __restrict__ d_volume) {
    __shared__ int s_cnt[MGB_MAX_S];
    __shared__ double s[4];
    const int b = blockIdx.x;
    const size_t row = (size_t)b * S;
    const int n_u = nu ? nu[b] : S;
    if (n_u <= 0) {                                   // empty frustum (the whole block takes this branch): exact zeros
        for (int u = threadIdx.x; u < S; u += 256) d_vis[row + u] = 0.f;
        if (d_volume && threadIdx.x == 0) d_volume[b] = 0.f;
        return;
    }
    const float cx = cam_world[3 * b], cy = cam_world[3 * b + 1], cz = cam_world[3 * b + 2];
    if (inv) {
        for (int u = threadIdx.x; u < S; u += 256) s_cnt[u] = 0;
        __syncthreads();
        for (int n = threadIdx.x; n < S; n += 256) {
            const long long u = inv[row + n];
            if (u >= 0 && u < S) atomicAdd(&s_cnt[u], 1);          // a bad index is skipped: nothing outside the counters is touched
        }
        __syncthreads();
    }
    const float scale = (g[b] * volume[b]) / (float)S;
    for (int u = threadIdx.x; u < S; u += 256) {
        const int c = u < n_u ? (inv ? s_cnt[u] : 1) : 0;
        float v = 0.f;
        if (c > 0) v = (scale * (float)c) * gain_distance_factor(world + (row + u) * pts_dim, cx, cy, cz, distance_th, mode);
        d_vis[row + u] = v;
    }
    if (!d_volume) return;
    double acc = 0.0;                                 // the forward's sum: over the samples in order, in double
    for (int n = threadIdx.x; n < S; n += 256) {
        const long long u = inv ? inv[row + n] : n;
        if (u < 0 || u >= S) continue;                // (skipped above as well)
        acc += (double)(vis[row + u] * gain_distance_factor(world + (row + u) * pts_dim, cx, cy, cz, distance_th, mode));
    }
    acc = wave_sum_all(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) d_volume[b] = g[b] * (float)(four_wave_sum(s) / (double)S);
}

}  // namespace mcr

using namespace mcr;

extern "C" int mcr_macarons_gain_backward(const float* grad_gains, const float* vis, const float* world, int pts_dim, const int64_t* inverse,
                                          const int* n_unique, const float* cam_world, const float* volume, float distance_th,
                                          int factor_mode, int64_t K, int S, float* d_vis, float* d_volume, void* stream) {
    MCR_REQUIRE(grad_gains && vis && world && cam_world && volume && d_vis && K > 0 && K <= 0x7fffffffll && S > 0 && pts_dim >= 3,
                "mcr_macarons_gain_backward: bad arguments");
    MCR_REQUIRE((inverse == nullptr) == (n_unique == nullptr),
                "mcr_macarons_gain_backward: inverse and n_unique go together (both NULL: the identity form)");
    MCR_REQUIRE(S <= MGB_MAX_S, "mcr_macarons_gain_backward: S = %d samples per camera, the limit is %d (one LDS counter each)", S, MGB_MAX_S);
    MCR_REQUIRE(factor_mode == 0 || factor_mode == 1, "mcr_macarons_gain_backward: factor_mode must be 0 (threshold) or 1 (smooth)");
    MCR_REQUIRE(distance_th > 0.f, "mcr_macarons_gain_backward: distance_th must be positive");
    hipLaunchKernelGGL(macarons_gain_bwd_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, grad_gains, vis, world, pts_dim,
                       (const long long*)inverse, n_unique, cam_world, volume, distance_th, factor_mode, S, d_vis, d_volume);
    MCR_LAUNCH_CHECK("macarons_gain_bwd_kernel");
    return 0;
}
