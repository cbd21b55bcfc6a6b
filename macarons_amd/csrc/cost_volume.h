// Device code shared by the plane sweep of the depth module (cost_volume.hip) and its backward (cost_volume_bwd.hip): the row
// butterfly, the bicubic tap of a lane, the pose of a source, the projection of a tap onto a plane and the bilinear corners of the
// resized coordinate.  Both directions run the sweep below, so both compute a coordinate with the same instructions.
#pragma once
#include "depth_geom.h"
#include "workspace.h"
#include <math.h>

namespace mcr {

constexpr int CV_C = 64;                             // feature channels: 16 lanes x float4
constexpr int CV_PLANES = 4;                         // depth planes per workgroup (126 VGPRs: four waves per SIMD; 8 planes need 231)
constexpr int CV_POS = 16;                           // output positions per workgroup (256 threads)

// Sum over the 16 lanes of a DPP row, the total in EVERY lane of the row with the same bits (each step adds the same two numbers in both
// partners): xor 1, xor 2 inside the quads, then the quads of a half mirrored, then the halves mirrored.
__device__ __forceinline__ float row16_sum_all(float v) {
    v += dpp_mov0<0xB1>(v);                          // quad_perm:[1,0,3,2]
    v += dpp_mov0<0x4E>(v);                          // quad_perm:[2,3,0,1]
    v += dpp_mov0<0x141>(v);                         // row_half_mirror
    v += dpp_mov0<0x140>(v);                         // row_mirror
    return v;
}

// Cubic convolution weight of tap r (0..3) at fraction t, A = -0.75 (upsample_bicubic2d's get_cubic_upsample_coefficients).
__device__ __forceinline__ double cubic_weight(double t, int r) {
    const double A = -0.75;
    const double x = r == 0 ? t + 1.0 : r == 1 ? t : r == 2 ? 1.0 - t : 2.0 - t;
    return (r == 0 || r == 3) ? ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A : ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
}

// The bilinear corners of a sample at pixel coordinate (px, py) of an Hf x Wf map: clamped pixel indices and weights; a corner outside
// the map, and every corner of a sample that is not `in`, has weight 0 (and the address of a pixel inside).
struct CvCorners {
    int x0c, x1c, y0c, y1c;
    float w00, w01, w10, w11;                        // nw ne sw se
};

__device__ __forceinline__ CvCorners cv_corners(float px, float py, bool in, int Hf, int Wf) {
    px = in ? px : 0.f;
    py = in ? py : 0.f;
    const float flx = floorf(px), fly = floorf(py);
    const int x0 = (int)flx, y0 = (int)fly;          // in [-1, size - 1]
    const float wx1 = px - flx, wx0 = (flx + 1.f) - px, wy1 = py - fly, wy0 = (fly + 1.f) - py;
    const bool x0in = in && x0 >= 0, x1in = in && x0 + 1 < Wf, y0in = y0 >= 0, y1in = y0 + 1 < Hf;
    CvCorners c;
    c.x0c = max(x0, 0), c.x1c = min(x0 + 1, Wf - 1), c.y0c = max(y0, 0), c.y1c = min(y0 + 1, Hf - 1);
    c.w00 = (x0in && y0in) ? wx0 * wy0 : 0.f, c.w01 = (x1in && y0in) ? wx1 * wy0 : 0.f;
    c.w10 = (x0in && y1in) ? wx0 * wy1 : 0.f, c.w11 = (x1in && y1in) ? wx1 * wy1 : 0.f;
    return c;
}

// What the backward keeps of a sample (b, a, k, p): the resized pixel coordinate the forward sampled at, bit for bit; px = CV_NOT_IN for
// a sample that failed the forward's `in` test (a coordinate that passes it is above -1).
constexpr float CV_NOT_IN = -2.f;

// The sweep of one row (16 lanes = one output position `pos`, lane l = bicubic tap l and channels 4l .. 4l+3) over the sources and the
// CV_PLANES planes from k0: acc[kk] = sum over the sources of the bilinear sample of channels 4l .. 4l+3 on plane k0 + kk.  Every lane of
// the row must call it (the butterflies).  RECORD: lane 0 also stores the sampled coordinate of every (source, plane) in
// samples[((b*A + a)*D + k)*P + pos] when `store` (a real position) and k < D.
template <bool RECORD>
__device__ __forceinline__ void cv_sweep_row(const float* __restrict__ xa_cl, const double* __restrict__ pose, const float* __restrict__ bins,
                                             float2* __restrict__ samples, int b, int k0, int pos, bool store, int lane, int A, int H, int W,
                                             int Hf, int Wf, int D, float fov_scale, float4 (&acc)[CV_PLANES]) {
    const int P = Hf * Wf;
    const int i = pos / Wf, j = pos - i * Wf;

    // ---- this lane's bicubic tap: full-resolution pixel (p, q), weight wy[r] * wx[c] (align_corners = False, indices clamped) ----
    const int r = lane >> 2, c = lane & 3;
    const double sy = (i + 0.5) * ((double)H / Hf) - 0.5, sx = (j + 0.5) * ((double)W / Wf) - 0.5;
    const double fy = floor(sy), fx = floor(sx);
    const int p = min(max((int)fy - 1 + r, 0), H - 1), q = min(max((int)fx - 1 + c, 0), W - 1);
    const float wgt = (float)(cubic_weight(sy - fy, r) * cubic_weight(sx - fx, c));
    const int mf = min(Hf, Wf);
    const double s = (double)fov_scale;
    double nx, ny;
    pixel_ray(H, W, fov_scale, p, q, nx, ny);
    const float cx = (float)(-((double)mf / Wf) * s), cy = (float)(-((double)mf / Hf) * s);

    float dk[CV_PLANES];
#pragma unroll
    for (int kk = 0; kk < CV_PLANES; ++kk) dk[kk] = bins[min(k0 + kk, D - 1)];   // planes past the end repeat the last one; not stored

#pragma unroll
    for (int kk = 0; kk < CV_PLANES; ++kk) acc[kk] = make_float4(0.f, 0.f, 0.f, 0.f);

    const float fWf = (float)Wf, fHf = (float)Hf;
    for (int a = 0; a < A; ++a) {
        const double* ps = pose + ((size_t)b * A + a) * 12;          // wave-uniform
        float u[3], t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[k] = (float)(nx * ps[k] + ny * ps[3 + k] + ps[6 + k]);
            t[k] = (float)ps[9 + k];
        }
        const float* base = xa_cl + ((size_t)b * A + a) * (size_t)P * CV_C + lane * 4;
#pragma unroll
        for (int kk = 0; kk < CV_PLANES; ++kk) {
            const float d = dk[kk];
            const float vx = fmaf(d, u[0], t[0]), vy = fmaf(d, u[1], t[1]), vz = fmaf(d, u[2], t[2]);
            const float aw = fmaxf(fabsf(vz), 1e-8f);
            const float w = vz < 0.f ? -aw : aw;     // sign(w) * max(|w|, eps), sign(0) taken as +1
            const float gx = row16_sum_all(wgt * ((cx * vx) / w));
            const float gy = row16_sum_all(wgt * ((cy * vy) / w));
            const float px = ((gx + 1.f) * fWf - 1.f) * 0.5f, py = ((gy + 1.f) * fHf - 1.f) * 0.5f;
            // decided in floating point, before any conversion: NaN, infinities and anything whose four corners all lie outside fail
            // this test and contribute zero (weights 0, address of pixel (0, 0))
            const bool in = px > -1.f && px < fWf && py > -1.f && py < fHf;
            if (RECORD) {
                if (lane == 0 && store && k0 + kk < D)
                    samples[(((size_t)b * A + a) * D + (k0 + kk)) * (size_t)P + pos] = make_float2(in ? px : CV_NOT_IN, in ? py : 0.f);
            }
            const CvCorners cn = cv_corners(px, py, in, Hf, Wf);
            const float4 f00 = *(const float4*)(base + ((size_t)cn.y0c * Wf + cn.x0c) * CV_C);
            const float4 f01 = *(const float4*)(base + ((size_t)cn.y0c * Wf + cn.x1c) * CV_C);
            const float4 f10 = *(const float4*)(base + ((size_t)cn.y1c * Wf + cn.x0c) * CV_C);
            const float4 f11 = *(const float4*)(base + ((size_t)cn.y1c * Wf + cn.x1c) * CV_C);
            acc[kk].x += ((f00.x * cn.w00 + f01.x * cn.w01) + f10.x * cn.w10) + f11.x * cn.w11;
            acc[kk].y += ((f00.y * cn.w00 + f01.y * cn.w01) + f10.y * cn.w10) + f11.y * cn.w11;
            acc[kk].z += ((f00.z * cn.w00 + f01.z * cn.w01) + f10.z * cn.w10) + f11.z * cn.w11;
            acc[kk].w += ((f00.w * cn.w00 + f01.w * cn.w01) + f10.w * cn.w10) + f11.w * cn.w11;
        }
    }
}

// The layout pass of cost_volume.hip: x_alpha [B*A,64,P] -> xa_cl [B*A,P,64] and the pose of every source (12 doubles each).
void cv_launch_channels_last(const float* x_alpha, float* xa_cl, int P, const float* cams, int64_t B, int A, double* pose, hipStream_t stream);

// The checks both entries share; `io` is the forward's out or the backward's d_out, `stride_name` what its batch stride is called.
inline int cv_check(const char* who, const void* x, const void* x_alpha, const void* cams, const void* depth_bins, const void* io,
                    const char* stride_name, int64_t batch_stride, int64_t B, int A, int C, int H, int W, int Hf, int Wf, int D, float fov_scale) {
    MCR_REQUIRE(x && x_alpha && cams && depth_bins && io, "%s: NULL operand", who);
    MCR_REQUIRE(C == CV_C, "%s: C = %d feature channels, only %d (ResNet layer1, upstream's feature extractor) is supported", who, C, CV_C);
    MCR_REQUIRE(B >= 1 && A >= 1 && D >= 1, "%s: B = %lld, A = %d, D = %d must all be at least 1", who, (long long)B, A, D);
    MCR_REQUIRE(Hf >= 1 && Wf >= 1 && Hf <= H && Wf <= W && H >= 2 && W >= 2,
                "%s: need 1 <= Hf <= H, 1 <= Wf <= W and H, W >= 2 (got image %d x %d, features %d x %d)", who, H, W, Hf, Wf);
    MCR_REQUIRE((int64_t)Hf * Wf <= 0x7fffffffll - CV_POS && (int64_t)H * W <= 0x7fffffffll, "%s: image too large for int pixel indices", who);
    MCR_REQUIRE(B <= 65535 && B * A <= 65535 && cdiv(D, CV_PLANES) <= 65535, "%s: B, B*A and D/%d are limited to 65535 (grid dimensions)", who,
                CV_PLANES);
    MCR_REQUIRE(batch_stride >= (int64_t)D * Hf * Wf, "%s: %s = %lld is less than D*Hf*Wf = %lld", who, stride_name, (long long)batch_stride,
                (long long)D * Hf * Wf);
    MCR_REQUIRE(fov_scale > 0.f && fov_scale < INFINITY, "%s: fov_scale = 1/tan(fov/2) must be positive and finite", who);
    return 0;
}

}  // namespace mcr
