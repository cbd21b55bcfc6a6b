// MCR_HIPCC_FLAGS: -ffp-contract=off
// The photometric reconstruction loss of the depth module (macarons/utility/macarons_utils.py:1091-1187 get_reconstruction_loss_fn, with
// reproject_depth_map / warp of ManyDepth.py:111-205 and SSIM of :809-842), fused, for gfx950 -- forward and backward.  The cameras are
// ground truth and the images are inputs: only the predicted depth carries a gradient, and that gradient is a gather per pixel.
//
// Per scale s, image b and pixel (p, q), with d = mask ? depth : zfar:
//   ray per unit depth  n = ((W/m - 2q/(m-1))/fov_scale, (H/m - 2p/(m-1))/fov_scale, 1), m = min(H, W)
//   source-view point   v = d u + t, u = n M, M = R^T R_a, t = T_a - T M      (the pose of cost_volume.hip)
//   w = sign(v_z) max(|v_z|, 1e-8);  grid g = (-(m/W) fov_scale v_x / w, -(m/H) fov_scale v_y / w)
//   Iw_a = bilinear sample of source a at g (align_corners = False, zeros or border padding)
//   l1_a = mean_c |I - Iw_a|;  ssim_a = mean_c clamp((1 - n/d)/2, 0, 1) over the 3x3 windows of the reflection-padded I and Iw_a
//   loss_a = f ssim_a + (1 - f) l1_a;  sel = min over a, the lowest index on a tie
//   loss[s] = sum_b sum_p sel mask / (sum_p mask + 1e-7) with a mask, the mean over B H W without one
//
// Forward, one launch for all scales and images (rl_forward_kernel): a workgroup owns a 16 x 16 tile of pixels and a one-pixel halo whose
// indices are reflected at the image border BEFORE the warp, so a halo value is the warped image at the reflected pixel, from that
// pixel's depth.  It warps every source into LDS (3 A floats a region pixel), holds the target beside it, forms the window statistics
// from LDS -- centred on the window's means, never as E[y^2] - mu^2 -- and stores one partial sum (and its mask count).  A second launch
// of one workgroup (rl_finish_kernel) adds the partials in a fixed order.  No floating-point atomics.
//
// Backward (rl_backward_kernel, after rl_mask_count_kernel with a mask): a gather per pixel that recomputes with the forward's own device
// code (this file is compiled without FMA contraction: the two directions see the same bits).  Inside the clamp
//   d ssim_n / d y_j = alpha_n + beta_n y_j + gamma_n x_j      per window n and channel, y the warped and x the target image,
// so a tile with a two-pixel halo gives the statistics of every window that touches the tile; a first LDS pass stores per window the
// three coefficients of its selected source times the window's gate (mask_n / mask_factor_b) d_loss[s] f/3, a second pass sums per pixel
// over every (window n, offset) whose reflected position is that pixel -- an edge pixel enters a window more than once -- and
//   d_depth[p] = sum_a sum_c dL/dIw[a,c,p] (dIw/dpx dpx/dd + dIw/dpy dpy/dd).
#include "depth_geom.h"
#include "workspace.h"
#include <math.h>

namespace mcr {

constexpr int RL_T = 16;                             // tile edge: 256 threads, one output pixel each
constexpr int RL_MAX_A = 8;                          // sources: the selected index fits a byte, LDS stays under 64 KiB
constexpr float RL_C1 = 1e-4f, RL_C2 = 9e-4f;        // 0.01^2, 0.03^2
constexpr int RL_NONE = 255;                         // "no window here" in the backward's index table
constexpr int RL_CNT_CHUNKS = 64;                    // workgroups that count an image's mask for the backward

struct RlArgs {
    const float* images;                             // [B,H,W,3]
    const float* alpha;                              // [B,A,H,W,3]
    const unsigned char* mask;                       // [B,H,W] or NULL
    const float* cams;                               // [B,1+A,12]
    const float* depth;                              // [S,B,H,W]
    int B, A, H, W, tiles_x;
    float fov_scale, zfar, f;
    int border;                                      // padding mode: 0 zeros, 1 border
};

__device__ __forceinline__ int rl_reflect(int c, int n) { return c < 0 ? -c : (c >= n ? 2 * n - 2 - c : c); }

// The poses of image b's sources into LDS, 12 doubles each (pose_column, depth_geom.h: the plane sweep's).
__device__ __forceinline__ void rl_pose(const float* __restrict__ cams, int b, int A, double* pose) {
    for (int i = threadIdx.x; i < 3 * A; i += blockDim.x) {
        const int a = i / 3, k = i - 3 * a;
        const float* cam0 = cams + (size_t)b * (1 + A) * 12;
        pose_column(cam0, cam0 + (size_t)(1 + a) * 12, k, pose + a * 12);
    }
}

// The warped value of the three channels of source image `src` [H,W,3] for the pixel whose ray is (nx, ny, 1) at depth d, and with GRAD
// its derivative with respect to d.  A coordinate that is not finite samples nothing, in either padding mode: value 0, gradient 0 and no
// address formed from it; `inside` is decided in floating point before any conversion.  Coordinates in double, samples in fp32.
template <bool GRAD>
__device__ __forceinline__ void rl_sample(const RlArgs& g, const float* __restrict__ src, const double* ps, double nx, double ny, float d,
                                          float (&val)[3], float (&dval)[3]) {
    // The coordinate chain runs in double: an fp32 pixel coordinate near 456 is spaced 3e-5 apart, that error times a steep image slope
    // is 1e-5 in the warped value, and d ssim / d y changes by about 100 per unit of y in flat windows -- 1e-3 of the gradient.
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = nx * ps[k] + ny * ps[3 + k] + ps[6 + k];
    const int H = g.H, W = g.W, m = min(H, W);
    const float fW = (float)W, fH = (float)H;
    const double cx = -((double)m / W) * (double)g.fov_scale, cy = -((double)m / H) * (double)g.fov_scale;
    const double dd = (double)d;
    const double vx = dd * u[0] + ps[9], vy = dd * u[1] + ps[10], vz = dd * u[2] + ps[11];
    const double aw = fmax(fabs(vz), 1e-8);
    const double w = vz < 0.0 ? -aw : aw;            // sign(w) * max(|w|, eps), sign(0) taken as +1
    const double iw = 1.0 / w;
    const double rx = vx * iw, ry = vy * iw;
    double pxd = ((cx * rx + 1.0) * (double)W - 1.0) * 0.5, pyd = ((cy * ry + 1.0) * (double)H - 1.0) * 0.5;
    // finite, inside and held are decided on the fp32 value of the coordinate: one that overflows fp32 is not finite
    const float pxf = (float)pxd, pyf = (float)pyd;
    bool in, movx = true, movy = true;               // mov: the pixel coordinate follows the grid coordinate (not held by border's clamp)
    if (g.border) {
        in = fabsf(pxf) < INFINITY && fabsf(pyf) < INFINITY;      // false for NaN
        movx = pxd > 0.0 && pxd < (double)(W - 1), movy = pyd > 0.0 && pyd < (double)(H - 1);
        pxd = fmin(fmax(pxd, 0.0), (double)(W - 1)), pyd = fmin(fmax(pyd, 0.0), (double)(H - 1));
    } else {
        in = pxf > -1.f && pxf < fW && pyf > -1.f && pyf < fH && pxd > -1.0 && pxd < (double)W && pyd > -1.0 && pyd < (double)H;
    }
    val[0] = val[1] = val[2] = 0.f;
    if (GRAD) dval[0] = dval[1] = dval[2] = 0.f;
    if (!in) return;
    const double flx = floor(pxd), fly = floor(pyd);
    const int x0 = (int)flx, y0 = (int)fly;          // in [-1, size - 1]
    const float wx1 = (float)(pxd - flx), wx0 = (float)((flx + 1.0) - pxd), wy1 = (float)(pyd - fly), wy0 = (float)((fly + 1.0) - pyd);
    const bool x0in = x0 >= 0, x1in = x0 + 1 < W, y0in = y0 >= 0, y1in = y0 + 1 < H;
    const int x0c = max(x0, 0), x1c = min(x0 + 1, W - 1), y0c = max(y0, 0), y1c = min(y0 + 1, H - 1);
    const float* p00 = src + ((size_t)y0c * W + x0c) * 3;
    const float* p01 = src + ((size_t)y0c * W + x1c) * 3;
    const float* p10 = src + ((size_t)y1c * W + x0c) * 3;
    const float* p11 = src + ((size_t)y1c * W + x1c) * 3;
    const bool i00 = x0in && y0in, i01 = x1in && y0in, i10 = x0in && y1in, i11 = x1in && y1in;
    float dpx = 0.f, dpy = 0.f;                      // d px / d depth, d py / d depth
    if (GRAD) {
        const double uz = fabs(vz) < 1e-8 ? 0.0 : u[2];          // the clamp holds w constant
        const double dgx = cx * ((u[0] - rx * uz) * iw), dgy = cy * ((u[1] - ry * uz) * iw);
        dpx = movx ? (float)(dgx * (double)W * 0.5) : 0.f, dpy = movy ? (float)(dgy * (double)H * 0.5) : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f00 = i00 ? p00[c] : 0.f, f01 = i01 ? p01[c] : 0.f, f10 = i10 ? p10[c] : 0.f, f11 = i11 ? p11[c] : 0.f;
        val[c] = ((f00 * (wx0 * wy0) + f01 * (wx1 * wy0)) + f10 * (wx0 * wy1)) + f11 * (wx1 * wy1);
        if (GRAD) {
            const float dvx = wy0 * (f01 - f00) + wy1 * (f11 - f10), dvy = wx0 * (f10 - f00) + wx1 * (f11 - f01);
            const float dv = dvx * dpx + dvy * dpy;
            dval[c] = fabsf(dv) < INFINITY ? dv : 0.f;
        }
    }
}

// The depth the warp of pixel (p, q) of (s, b) uses.
__device__ __forceinline__ float rl_depth(const RlArgs& g, int s, int b, int p, int q) {
    const size_t pix = ((size_t)b * g.H + p) * g.W + q;
    const float d = g.depth[(size_t)s * g.B * g.H * g.W + pix];
    return (g.mask && !g.mask[pix]) ? g.zfar : d;
}

// Fills the region of a tile: padded coordinates [y0 - HALO, y0 + RL_T + HALO) x [x0 - HALO, ...), row-major, RW = RL_T + 2 HALO wide.
// tgt[c * R + r] the target, wrp[(a * 3 + c) * R + r] the warped sources, at the REFLECTED pixel of r; a padded coordinate outside
// [-1, size] belongs to no window and holds 0.
template <int HALO>
__device__ __forceinline__ void rl_warp_region(const RlArgs& g, int s, int b, int y0, int x0, const double* pose, float* tgt, float* wrp) {
    constexpr int RW = RL_T + 2 * HALO, R = RW * RW;
    const int H = g.H, W = g.W, A = g.A;
    for (int r = threadIdx.x; r < R; r += RL_T * RL_T) {
        const int ry = r / RW, rx = r - ry * RW;
        const int cyp = y0 - HALO + ry, cxp = x0 - HALO + rx;
        const bool used = cyp >= -1 && cyp <= H && cxp >= -1 && cxp <= W;
        if (!used) {
#pragma unroll
            for (int c = 0; c < 3; ++c) tgt[c * R + r] = 0.f;
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) wrp[(a * 3 + c) * R + r] = 0.f;
            continue;
        }
        const int p = rl_reflect(cyp, H), q = rl_reflect(cxp, W);
        const float* ip = g.images + (((size_t)b * H + p) * W + q) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) tgt[c * R + r] = ip[c];
        const float d = rl_depth(g, s, b, p, q);
        double nx, ny;
        pixel_ray(g.H, g.W, g.fov_scale, p, q, nx, ny);
        for (int a = 0; a < A; ++a) {
            float val[3], dval[3];
            rl_sample<false>(g, g.alpha + ((size_t)b * A + a) * (size_t)H * W * 3, pose + a * 12, nx, ny, d, val, dval);
#pragma unroll
            for (int c = 0; c < 3; ++c) wrp[(a * 3 + c) * R + r] = val[c];
        }
    }
}

// loss_a of the window centred on region index r (RW wide, R per channel plane), from LDS.  COEF: also co[3 c + 0..2] = alpha, beta, gamma
// of d ssim_c / d y_j = alpha + beta y_j + gamma x_j (all 0 outside the clamp).
template <bool COEF>
__device__ __forceinline__ float rl_window_loss(const float* tgt, const float* wrp_a, int r, int RW, int R, float f, float (&co)[9]) {
    float l1 = 0.f, ss = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) l1 += fabsf(tgt[c * R + r] - wrp_a[c * R + r]);
    l1 = l1 / 3.f;
    if (!(f > 0.f)) return l1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* xp = tgt + c * R + r - RW - 1;
        const float* yp = wrp_a + c * R + r - RW - 1;
        float x[9], y[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) x[3 * i + j] = xp[i * RW + j], y[3 * i + j] = yp[i * RW + j];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) sx += x[i], sy += y[i];
        const float mx = sx / 9.f, my = sy / 9.f;
        float vxx = 0.f, vyy = 0.f, vxy = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float dx = x[i] - mx, dy = y[i] - my;
            vxx += dx * dx, vyy += dy * dy, vxy += dx * dy;
        }
        const float a1 = 2.f * mx * my + RL_C1, a2 = 2.f * (vxy / 9.f) + RL_C2;
        const float b1 = mx * mx + my * my + RL_C1, b2 = (vxx / 9.f + vyy / 9.f) + RL_C2;
        const float den = b1 * b2;
        const float ratio = (a1 * a2) / den;
        const float raw = (1.f - ratio) * 0.5f;
        ss += fminf(fmaxf(raw, 0.f), 1.f);
        if (COEF) {
            const bool open = raw >= 0.f && raw <= 1.f;           // torch's clamp backward
            const float k = -1.f / (9.f * den);
            co[3 * c + 0] = open ? k * (mx * (a2 - a1) - ratio * my * (b2 - b1)) : 0.f;
            co[3 * c + 1] = open ? -k * ratio * b1 : 0.f;
            co[3 * c + 2] = open ? k * a1 : 0.f;
        }
    }
    return f * (ss / 3.f) + (1.f - f) * l1;
}

// The selected loss and index of the window at region index r: the min over the sources, the lowest index on a tie.
__device__ __forceinline__ float rl_select(const float* tgt, const float* wrp, int r, int RW, int R, int A, float f, int& sel) {
    float best = 0.f, co[9];
    sel = 0;
    for (int a = 0; a < A; ++a) {
        const float l = rl_window_loss<false>(tgt, wrp + (size_t)a * 3 * R, r, RW, R, f, co);
        if (a == 0 || l < best) best = l, sel = a;
    }
    return best;
}

__global__ __launch_bounds__(RL_T* RL_T) void rl_forward_kernel(RlArgs g, float* __restrict__ loss_map, unsigned char* __restrict__ argmin,
                                                               float* __restrict__ part_sum, int* __restrict__ part_cnt) {
    constexpr int HALO = 1, RW = RL_T + 2 * HALO, R = RW * RW;
    extern __shared__ __align__(16) unsigned char rl_lds[];
    double* pose = (double*)rl_lds;                                  // [A,12]
    float* tgt = (float*)(pose + 12 * g.A);                          // [3,R]
    float* wrp = tgt + 3 * R;                                        // [A,3,R]
    __shared__ float red[4];
    __shared__ int redc[4];
    const int tile = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
    const int y0 = (tile / g.tiles_x) * RL_T, x0 = (tile % g.tiles_x) * RL_T;
    rl_pose(g.cams, b, g.A, pose);
    __syncthreads();
    rl_warp_region<HALO>(g, s, b, y0, x0, pose, tgt, wrp);
    __syncthreads();
    const int ty = threadIdx.x / RL_T, tx = threadIdx.x % RL_T;
    const int p = y0 + ty, q = x0 + tx;
    float contrib = 0.f;
    int cnt = 0;
    if (p < g.H && q < g.W) {
        int sel;
        const float l = rl_select(tgt, wrp, (ty + HALO) * RW + tx + HALO, RW, R, g.A, g.f, sel);
        const size_t pix = ((size_t)b * g.H + p) * g.W + q, o = (size_t)s * g.B * g.H * g.W + pix;
        if (loss_map) loss_map[o] = l;
        if (argmin) argmin[o] = (unsigned char)sel;
        const bool on = !g.mask || g.mask[pix];
        contrib = on ? l : 0.f, cnt = on ? 1 : 0;
    }
    const float tot = block_sum_256(contrib, red);
    cnt = block_sum_256(cnt, redc);
    if (threadIdx.x == 0) {
        const size_t i = ((size_t)s * g.B + b) * gridDim.x + tile;
        part_sum[i] = tot, part_cnt[i] = cnt;
    }
}

// One workgroup: a wave per (s, b) adds that image's partials in a fixed order; then a thread per scale adds the images, ascending.
__global__ __launch_bounds__(256) void rl_finish_kernel(const float* __restrict__ part_sum, const int* __restrict__ part_cnt,
                                                        double* __restrict__ sb, float* __restrict__ loss, int S, int B, int n_tiles,
                                                        int masked, double n_pixels) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = wave; i < (int64_t)S * B; i += 4) {
        double acc = 0.0;
        long long c = 0;
        for (int t = lane; t < n_tiles; t += 64) acc += (double)part_sum[i * n_tiles + t], c += part_cnt[i * n_tiles + t];
        acc = wave_sum_all(acc), c = wave_sum_all(c);
        if (lane == 0) sb[i] = masked ? acc / (double)((float)c + 1e-7f) : acc;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += sb[(int64_t)s * B + b];
        loss[s] = (float)(masked ? acc : acc / n_pixels);
    }
}

// cnt[b * RL_CNT_CHUNKS + c] = the number of set mask pixels in chunk c of image b: integers, one workgroup a chunk; the backward adds an
// image's chunks itself (one workgroup an image took 28 us of the backward's 104 at 256 x 456).
__global__ __launch_bounds__(256) void rl_mask_count_kernel(const unsigned char* __restrict__ mask, int64_t n_pix, int* __restrict__ cnt) {
    __shared__ int red[4];
    const unsigned char* mb = mask + (size_t)blockIdx.y * n_pix;
    int64_t i0, i1;
    chunk_range(n_pix, RL_CNT_CHUNKS, blockIdx.x, i0, i1);
    int c = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) c += mb[i] ? 1 : 0;
    c = block_sum_256(c, red);
    if (threadIdx.x == 0) cnt[blockIdx.y * RL_CNT_CHUNKS + blockIdx.x] = c;
}

__global__ __launch_bounds__(RL_T* RL_T) void rl_backward_kernel(RlArgs g, const float* __restrict__ d_loss, const int* __restrict__ mask_cnt,
                                                                float* __restrict__ d_depth) {
    constexpr int HALO = 2, RW = RL_T + 2 * HALO, R = RW * RW;      // the region of warped values
    constexpr int NW = RL_T + 2, N = NW * NW;                        // the window centres: the tile and one pixel around it
    extern __shared__ __align__(16) unsigned char rl_lds[];
    double* pose = (double*)rl_lds;                                  // [A,12]
    float* tgt = (float*)(pose + 12 * g.A);                          // [3,R]
    float* wrp = tgt + 3 * R;                                        // [A,3,R]
    float* coef = wrp + (size_t)g.A * 3 * R;                         // [9,N]: alpha, beta, gamma per channel of the selected source, gated
    float* gate = coef + 9 * N;                                      // [N]: the window's own gate (its L1 term)
    int* wsel = (int*)(gate + N);                                    // [N]: the selected source, RL_NONE where no window is
    const int tile = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
    const int y0 = (tile / g.tiles_x) * RL_T, x0 = (tile % g.tiles_x) * RL_T;
    const int H = g.H, W = g.W, A = g.A;
    rl_pose(g.cams, b, A, pose);
    __syncthreads();
    rl_warp_region<HALO>(g, s, b, y0, x0, pose, tgt, wrp);
    __syncthreads();
    const float dl = d_loss[s];
    int cnt = 0;
    if (g.mask)
        for (int i = 0; i < RL_CNT_CHUNKS; ++i) cnt += mask_cnt[b * RL_CNT_CHUNKS + i];
    const float norm = g.mask ? 1.f / ((float)cnt + 1e-7f) : (float)(1.0 / ((double)g.B * H * W));
    for (int n = threadIdx.x; n < N; n += RL_T * RL_T) {
        const int wy = n / NW, wx = n - wy * NW;
        const int p = y0 - 1 + wy, q = x0 - 1 + wx;
        float co[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) co[i] = 0.f;
        int sel = RL_NONE;
        float gt = 0.f;
        if (p >= 0 && p < H && q >= 0 && q < W) {
            const int r = (wy + 1) * RW + wx + 1;
            rl_select(tgt, wrp, r, RW, R, A, g.f, sel);
            const bool on = !g.mask || g.mask[((size_t)b * H + p) * W + q];
            gt = on ? norm * dl : 0.f;
            if (g.f > 0.f && on) {
                rl_window_loss<true>(tgt, wrp + (size_t)sel * 3 * R, r, RW, R, g.f, co);
                const float gs = gt * (g.f / 3.f);
#pragma unroll
                for (int i = 0; i < 9; ++i) co[i] *= gs;
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) coef[i * N + n] = co[i];
        gate[n] = gt, wsel[n] = sel;
    }
    __syncthreads();
    const int ty = threadIdx.x / RL_T, tx = threadIdx.x % RL_T;
    const int p = y0 + ty, q = x0 + tx;
    if (p >= H || q >= W) return;
    const size_t pix = ((size_t)b * H + p) * W + q, o = (size_t)s * g.B * H * W + pix;
    if (g.mask && !g.mask[pix]) {                                    // warped at zfar, a constant
        d_depth[o] = 0.f;
        return;
    }
    // the padded positions that reflect onto this pixel, per axis: itself, -1 for pixel 1, size for pixel size - 2
    int cys[3], cxs[3], ncy = 0, ncx = 0;
    cys[ncy++] = p;
    if (p == 1) cys[ncy++] = -1;
    if (p == H - 2) cys[ncy++] = H;
    cxs[ncx++] = q;
    if (q == 1) cxs[ncx++] = -1;
    if (q == W - 2) cxs[ncx++] = W;
    const int rc = (ty + HALO) * RW + tx + HALO, nc = (ty + 1) * NW + tx + 1;
    const float d = g.depth[o];
    double nx, ny;
    pixel_ray(H, W, g.fov_scale, p, q, nx, ny);
    float acc = 0.f;
    for (int a = 0; a < A; ++a) {
        float ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f}, cg[3] = {0.f, 0.f, 0.f};
        bool any = false;
        if (g.f > 0.f) {
            for (int iy = 0; iy < ncy; ++iy)
                for (int dy = -1; dy <= 1; ++dy) {
                    const int np_ = cys[iy] - dy;
                    if (np_ < 0 || np_ >= H) continue;
                    for (int ix = 0; ix < ncx; ++ix)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int nq = cxs[ix] - dx;
                            if (nq < 0 || nq >= W) continue;
                            const int n = (np_ - (y0 - 1)) * NW + (nq - (x0 - 1));       // |np_ - p| <= 1 and |nq - q| <= 1: inside the table
                            if (wsel[n] != a) continue;
                            any = true;
#pragma unroll
                            for (int c = 0; c < 3; ++c) ca[c] += coef[(3 * c + 0) * N + n], cb[c] += coef[(3 * c + 1) * N + n], cg[c] += coef[(3 * c + 2) * N + n];
                        }
                }
        }
        const bool own = wsel[nc] == a;
        if (!any && !own) continue;
        float val[3], dval[3];
        rl_sample<true>(g, g.alpha + ((size_t)b * A + a) * (size_t)H * W * 3, pose + a * 12, nx, ny, d, val, dval);
        const float gl1 = own ? gate[nc] * ((1.f - g.f) / 3.f) : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = tgt[c * R + rc], y = wrp[(a * 3 + c) * R + rc];
            const float diff = x - y;
            const float sg = diff > 0.f ? -1.f : (diff < 0.f ? 1.f : 0.f);               // d |x - y| / dy, sign(0) = 0
            acc += ((ca[c] + cb[c] * y + cg[c] * x) + gl1 * sg) * dval[c];
        }
    }
    d_depth[o] = acc;
}

static bool rl_sizes_ok(int64_t S, int64_t B, int64_t A, int64_t H, int64_t W) {
    if (S < 1 || B < 1 || A < 1 || A > RL_MAX_A || H < 2 || W < 2) return false;
    if (S > 65535 || B > 65535) return false;                                           // grid dimensions
    if (H > 0x3fffffffll || W > 0x3fffffffll || H * W > 0x7fffffffll - 4 * RL_T * RL_T) return false;   // int pixel indices
    if ((double)S * (double)B * (double)cdiv(H, RL_T) * (double)cdiv(W, RL_T) > 2147483647.0) return false;   // the partials
    if ((double)S * (double)B * (double)A * (double)H * (double)W * 12.0 > 9.0e18) return false;        // byte offsets
    return true;
}

// The forward's workspace: a partial sum and a mask count per (s, b, tile), a double per (s, b).
struct RlFwdScratch { float* part_sum; int* part_cnt; double* sb; };
static RlFwdScratch carve_rl_fwd(Arena& a, int64_t S, int64_t B, int64_t H, int64_t W) {
    const size_t n = (size_t)S * B * (size_t)(cdiv(H, RL_T) * cdiv(W, RL_T));
    RlFwdScratch w;
    w.part_sum = a.f(n);
    w.part_cnt = (int*)a.bytes(n * sizeof(int));
    w.sb = (double*)a.bytes((size_t)S * B * sizeof(double));
    return w;
}

// The backward's: the mask counts of every image, by chunk.
struct RlBwdScratch { int* mask_cnt; };
static RlBwdScratch carve_rl_bwd(Arena& a, int64_t B) { return {(int*)a.bytes((size_t)B * RL_CNT_CHUNKS * sizeof(int))}; }

static int rl_check(const char* who, const void* images, const void* alpha, const void* cams, const void* depth, int64_t S, int64_t B, int A,
                    int H, int W, float fov_scale, float zfar, float ssim_factor, int padding_mode) {
    MCR_REQUIRE(images && alpha && cams && depth, "%s: NULL operand", who);
    MCR_REQUIRE(A >= 1 && A <= RL_MAX_A, "%s: A = %d sources, 1 .. %d are supported (the selected index is a byte)", who, A, RL_MAX_A);
    MCR_REQUIRE(H >= 2 && W >= 2, "%s: the image is %d x %d, H and W must be at least 2 (the reflection padding)", who, H, W);
    MCR_REQUIRE(S >= 1 && B >= 1, "%s: S = %lld, B = %lld must be at least 1", who, (long long)S, (long long)B);
    MCR_REQUIRE(padding_mode == 0 || padding_mode == 1, "%s: padding mode %d, only 0 (zeros) and 1 (border) are supported", who, padding_mode);
    MCR_REQUIRE(rl_sizes_ok(S, B, A, H, W), "%s: S = %lld, B = %lld, A = %d, %d x %d: a product of the sizes overflows an index", who,
                (long long)S, (long long)B, A, H, W);
    MCR_REQUIRE(fov_scale > 0.f && fov_scale < INFINITY, "%s: fov_scale = 1/tan(fov/2) must be positive and finite", who);
    MCR_REQUIRE(fabsf(zfar) < INFINITY, "%s: zfar must be finite", who);
    MCR_REQUIRE(ssim_factor >= 0.f && ssim_factor <= 1.f, "%s: ssim_factor = %g must lie in [0, 1]", who, (double)ssim_factor);
    return 0;
}

static RlArgs rl_args(const float* images, const float* alpha, const unsigned char* mask, const float* cams, const float* depth, int64_t B,
                      int A, int H, int W, float fov_scale, float zfar, float ssim_factor, int padding_mode) {
    RlArgs g;
    g.images = images, g.alpha = alpha, g.mask = mask, g.cams = cams, g.depth = depth;
    g.B = (int)B, g.A = A, g.H = H, g.W = W, g.tiles_x = (int)cdiv(W, RL_T);
    g.fov_scale = fov_scale, g.zfar = zfar, g.f = ssim_factor, g.border = padding_mode;
    return g;
}

}  // namespace mcr

using namespace mcr;

extern "C" size_t mcr_reconstruction_loss_workspace_bytes(int64_t S, int64_t B, int64_t A, int64_t H, int64_t W) {
    if (!rl_sizes_ok(S, B, A, H, W)) return 0;
    return measure(carve_rl_fwd, S, B, H, W);
}

extern "C" int mcr_reconstruction_loss(const float* images, const float* alpha_images, const unsigned char* mask, const float* cams,
                                       const float* depth, float* loss, float* loss_map, unsigned char* argmin, int64_t S, int64_t B, int A,
                                       int H, int W, float fov_scale, float zfar, float ssim_factor, int padding_mode, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const char* who = "mcr_reconstruction_loss";
    if (int e = rl_check(who, images, alpha_images, cams, depth, S, B, A, H, W, fov_scale, zfar, ssim_factor, padding_mode)) return e;
    MCR_REQUIRE(loss, "%s: NULL loss", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_reconstruction_loss_workspace_bytes(S, B, A, H, W))) return e;

    const hipStream_t st = (hipStream_t)stream;
    Arena arena{(char*)workspace, workspace_bytes};
    const RlFwdScratch ws = carve_rl_fwd(arena, S, B, H, W);
    const RlArgs g = rl_args(images, alpha_images, mask, cams, depth, B, A, H, W, fov_scale, zfar, ssim_factor, padding_mode);
    const int n_tiles = (int)(cdiv(H, RL_T) * cdiv(W, RL_T));
    constexpr int R = (RL_T + 2) * (RL_T + 2);
    const size_t lds = (size_t)A * 12 * sizeof(double) + (size_t)(3 + 3 * A) * R * sizeof(float);
    hipLaunchKernelGGL(rl_forward_kernel, dim3((unsigned)n_tiles, (unsigned)B, (unsigned)S), dim3(RL_T * RL_T), lds, st, g, loss_map, argmin,
                       ws.part_sum, ws.part_cnt);
    MCR_LAUNCH_CHECK("rl_forward_kernel");
    hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(256), 0, st, ws.part_sum, ws.part_cnt, ws.sb, loss, (int)S, (int)B, n_tiles, mask ? 1 : 0,
                       (double)B * H * W);
    MCR_LAUNCH_CHECK("rl_finish_kernel");
    return 0;
}

extern "C" size_t mcr_reconstruction_loss_backward_workspace_bytes(int64_t S, int64_t B, int64_t A, int64_t H, int64_t W) {
    if (!rl_sizes_ok(S, B, A, H, W)) return 0;
    return measure(carve_rl_bwd, B);
}

extern "C" int mcr_reconstruction_loss_backward(const float* images, const float* alpha_images, const unsigned char* mask, const float* cams,
                                                const float* depth, const float* d_loss, float* d_depth, int64_t S, int64_t B, int A, int H,
                                                int W, float fov_scale, float zfar, float ssim_factor, int padding_mode, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    const char* who = "mcr_reconstruction_loss_backward";
    if (int e = rl_check(who, images, alpha_images, cams, depth, S, B, A, H, W, fov_scale, zfar, ssim_factor, padding_mode)) return e;
    MCR_REQUIRE(d_loss && d_depth, "%s: NULL d_loss or d_depth", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_reconstruction_loss_backward_workspace_bytes(S, B, A, H, W))) return e;

    const hipStream_t st = (hipStream_t)stream;
    Arena arena{(char*)workspace, workspace_bytes};
    int* mask_cnt = carve_rl_bwd(arena, B).mask_cnt;
    const RlArgs g = rl_args(images, alpha_images, mask, cams, depth, B, A, H, W, fov_scale, zfar, ssim_factor, padding_mode);
    if (mask) {
        hipLaunchKernelGGL(rl_mask_count_kernel, dim3(RL_CNT_CHUNKS, (unsigned)B), dim3(256), 0, st, mask, (int64_t)H * W, mask_cnt);
        MCR_LAUNCH_CHECK("rl_mask_count_kernel");
    }
    const int n_tiles = (int)(cdiv(H, RL_T) * cdiv(W, RL_T));
    constexpr int R = (RL_T + 4) * (RL_T + 4), N = (RL_T + 2) * (RL_T + 2);
    const size_t lds = (size_t)A * 12 * sizeof(double) + (size_t)(3 + 3 * A) * R * sizeof(float) + (size_t)N * (10 * sizeof(float) + sizeof(int));
    hipLaunchKernelGGL(rl_backward_kernel, dim3((unsigned)n_tiles, (unsigned)B, (unsigned)S), dim3(RL_T * RL_T), lds, st, g, d_loss, mask_cnt,
                       d_depth);
    MCR_LAUNCH_CHECK("rl_backward_kernel");
    return 0;
}
