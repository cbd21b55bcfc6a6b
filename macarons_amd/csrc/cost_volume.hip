// Plane-sweep cost volume of the depth module (CostVolumeBuilder.forward, macarons/networks/ManyDepth.py:207-305) for gfx950, fused:
// unprojection of the full-resolution pixel grid at every depth plane, projection into every source camera, the bicubic resize of the
// projected coordinates to the feature resolution, the bilinear grid_sample of the source features, the mean over the sources and the
// L1 distance to the target features -- without any of upstream's intermediates (B*D*A cameras, B*D*H*W*3 world points per source, D
// copies of the source feature maps, the [B,D,A,C,Hf,Wf] warped tensor).
//
// What makes it cheap:
//   * the source-view point of a full-resolution pixel is affine in the plane depth d:  v = d * u + t,  u = n (R^T R_a),
//     t = T_a - T (R^T R_a),  n = (ndc_x / s, ndc_y / s, 1)  (u per bicubic tap and source, t per source; both set up in double, R^T R_a
//     and t once per source by the layout kernel);
//   * an output position has 4 x 4 bicubic taps and C = 64 channels: SIXTEEN LANES (one DPP row) own it -- lane l projects tap l and
//     gathers channels 4l .. 4l+3.  The 16 weighted tap coordinates are summed over the row (every lane ends with the same bits), and the
//     bilinear corners are then one contiguous 256-B read per row from a channels-last copy of the source maps (made here, in the
//     workspace; at upstream's size both maps fit one XCD's L2);
//   * a workgroup is 16 consecutive positions x 4 planes; the accumulators of the 4 planes stay in registers while the sources are swept,
//     the 4 chains are independent (branch-free: outside corners are read at a clamped address with weight 0) and hide each other's
//     latency.
// No atomics; every sum has a fixed order (sources ascending, corners nw ne sw se, the row butterflies), so two runs give the same bits.
#include "cost_volume.h"

namespace mcr {

// [img, 64, P] -> [img, P, 64] through a 64 x 64 LDS tile (padded: the transposed read is conflict-free).  The first workgroup of an
// image (b, a) also writes its pose, 12 doubles (pose_column, depth_geom.h).
__global__ __launch_bounds__(256) void cv_channels_last_kernel(const float* __restrict__ src, float* __restrict__ dst, int P,
                                                               const float* __restrict__ cams, int A, double* __restrict__ pose) {
    __shared__ float tile[CV_C][CV_C + 1];
    const int64_t img = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        const float* cam0 = cams + (img / A) * (1 + A) * 12;
        pose_column(cam0, cam0 + (1 + img % A) * 12, threadIdx.x, pose + img * 12);
    }
    const int p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c = ty; c < CV_C; c += 4) {
        const int p = p0 + tx;
        tile[c][tx] = p < P ? src[(img * CV_C + c) * P + p] : 0.f;
    }
    __syncthreads();
    for (int pp = ty; pp < 64; pp += 4) {
        const int p = p0 + pp;
        if (p < P) dst[(img * P + p) * CV_C + tx] = tile[tx][pp];
    }
}

__global__ __launch_bounds__(256) void cv_sweep_kernel(const float* __restrict__ x, const float* __restrict__ xa_cl,
                                                       const double* __restrict__ pose, const float* __restrict__ bins,
                                                       float* __restrict__ out, int64_t out_batch_stride, int A, int H, int W, int Hf, int Wf,
                                                       int D, float fov_scale) {
    const int lane = threadIdx.x & 15;
    const int P = Hf * Wf;
    const int pos_raw = blockIdx.x * CV_POS + (threadIdx.x >> 4);
    const bool valid = pos_raw < P;
    const int pos = valid ? pos_raw : P - 1;          // a row past the end repeats the last position (every lane stays in the butterflies)
    const int b = blockIdx.z;
    const int k0 = blockIdx.y * CV_PLANES;
    float4 acc[CV_PLANES];
    cv_sweep_row<false>(xa_cl, pose, bins, nullptr, b, k0, pos, valid, lane, A, H, W, Hf, Wf, D, fov_scale, acc);

    // ---- mean over the sources, L1 distance to the target features over the 64 channels ----
    const float* xt = x + ((size_t)b * CV_C + lane * 4) * (size_t)P + pos;
    const float x0v = xt[0], x1v = xt[P], x2v = xt[2 * (size_t)P], x3v = xt[3 * (size_t)P];
    const float inv_a = 1.f / (float)A;
#pragma unroll
    for (int kk = 0; kk < CV_PLANES; ++kk) {
        const float part = (fabsf(acc[kk].x * inv_a - x0v) + fabsf(acc[kk].y * inv_a - x1v)) +
                           (fabsf(acc[kk].z * inv_a - x2v) + fabsf(acc[kk].w * inv_a - x3v));
        const float tot = row16_sum_all(part);
        if (lane == 0 && valid && k0 + kk < D) out[(size_t)b * out_batch_stride + (size_t)(k0 + kk) * P + pos] = tot * (1.f / CV_C);
    }
}

void cv_launch_channels_last(const float* x_alpha, float* xa_cl, int P, const float* cams, int64_t B, int A, double* pose, hipStream_t stream) {
    hipLaunchKernelGGL(cv_channels_last_kernel, dim3((unsigned)cdiv(P, 64), (unsigned)(B * A)), dim3(256), 0, stream, x_alpha, xa_cl, P, cams, A,
                       pose);
}

}  // namespace mcr

using namespace mcr;

// channels-last copy of the source maps | poses
struct CvScratch { float* xa_cl; double* pose; };
static CvScratch carve_cv(Arena& a, int64_t B, int64_t A, int64_t C, int64_t P) {
    CvScratch w;
    w.xa_cl = a.f((size_t)B * A * C * P);
    w.pose = (double*)a.bytes((size_t)B * A * 12 * sizeof(double));
    return w;
}

extern "C" size_t mcr_cost_volume_workspace_bytes(int64_t B, int64_t A, int64_t C, int64_t Hf, int64_t Wf) {
    if (B <= 0 || A <= 0 || C <= 0 || Hf <= 0 || Wf <= 0) return 0;
    return measure(carve_cv, B, A, C, Hf * Wf);
}

extern "C" int mcr_cost_volume(const float* x, const float* x_alpha, const float* cams, const float* depth_bins, float* out,
                               int64_t out_batch_stride, int64_t B, int A, int C, int H, int W, int Hf, int Wf, int D, float fov_scale,
                               void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_cost_volume";
    if (int e = cv_check(who, x, x_alpha, cams, depth_bins, out, "out_batch_stride", out_batch_stride, B, A, C, H, W, Hf, Wf, D, fov_scale)) return e;
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_cost_volume_workspace_bytes(B, A, C, Hf, Wf))) return e;
    const int P = Hf * Wf;
    Arena arena{(char*)workspace, workspace_bytes};
    const CvScratch ws = carve_cv(arena, B, A, C, P);
    cv_launch_channels_last(x_alpha, ws.xa_cl, P, cams, B, A, ws.pose, (hipStream_t)stream);
    MCR_LAUNCH_CHECK("cv_channels_last_kernel");
    hipLaunchKernelGGL(cv_sweep_kernel, dim3((unsigned)cdiv(P, CV_POS), (unsigned)cdiv(D, CV_PLANES), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, ws.xa_cl, ws.pose, depth_bins, out, out_batch_stride, A, H, W, Hf, Wf, D, fov_scale);
    MCR_LAUNCH_CHECK("cv_sweep_kernel");
    return 0;
}
