// The disparity heads of the depth decoder (macarons/networks/ManyDepth.py:366-384 DisparityLayer: a reflection pad, a 3 x 3 convolution to
// ONE output channel and a sigmoid; disp1..disp4 of the decoder, :442-472), fused, for gfx950 -- forward and backward.  With one output
// channel there is no GEMM in it: it is a memory-bound stencil over x [B,C,Hs,Ws].
//
//   z[b,i,j] = bias + sum_c sum_{di,dj in -1..1} weight[c,di+1,dj+1] x[b,c,r(i+di,Hs),r(j+dj,Ws)],   r(-1,n) = 1, r(n,n) = n-2 (torch's reflect)
//   y = 1 / (1 + exp(-z))
//
// Forward, one launch: dh_forward_kernel.  A workgroup of 256 threads owns a tile of one image for all channels, a thread one pixel.  A
// pass of channels at a time the tile and its one-pixel ring go to LDS, rows along W, the ring reflected by index at the image's border
// (no padded copy exists); every pixel's thread then adds its 9 products per channel, c ascending, the taps row-major, starting from the
// bias.  A pass travels through registers with all of a thread's loads in flight at once, and the next pass is loaded while this one is
// added: with one load waited for at a time a pass costs as many memory latencies as a thread has loads.  The weights are
// wave-uniform: the compiler reads them with scalar loads through the constant cache, once per wave and never per thread.  The tile is
// 32 x 8 in passes of 8 channels, or 16 x 4 in passes of 24 -- one wave adds, all four stage -- where the larger tile would give the machine
// fewer workgroups than it has compute units (upstream's scales 2 to 4 at B = 1: scale 4 is 32 x 57 pixels against 128 channels).
//
// Backward.  With g = d_y y (1 - y) (y is an input) and g0 its extension by zeros, the loss is bilinear in weight and x,
//   sum_q g[q] z[q] = sum_c sum_t weight[c,t] sum_p x[b,c,p] S_t[b,p] + bias sum g,
//   S_t[b,p] = the sum of g0 over the output pixels q whose tap t reads pixel p, through the reflection included:
// along one axis pixel i is read through tap d by q = i - d, and besides, as the mirror image of padded row -1, by q = 0 through tap -1
// when i = 1, and as the image of padded row n by q = n - 1 through tap +1 when i = n - 2 (both at once when n = 3; on a two-pixel axis the
// two mirrors land on different pixels).  The two axes multiply: up to four output pixels per tap.  S does not depend on the channel, so
//   d_x[b,c,p] = sum_t weight[c,t] S_t[b,p]          dh_backward_x_kernel: a gather; x is not read at all
//   d_weight[c,t] = sum_{b,p} x[b,c,p] S_t[b,p]      dh_backward_w_kernel: x is read once, at the pixel itself, no ring
//   d_bias = sum g
// Both kernels hold g of the tile and its ring in LDS (zero outside the image, plus one zero cell that absent sources point to) and form
// the nine S_t of a pixel in registers, each as (g + g) + (g + g).  dh_backward_w_kernel: a workgroup owns a 64 x 16 tile of one image
// and DH_CG channels, a thread four pixels; it keeps the 9 DH_CG sums in registers over its pixels, the workgroup adds them in the fixed
// order of common.h and stores ONE partial per sum (slot b tiles + tile); dh_backward_finish_kernel adds the partials of an output, a wave
// per output, the lanes over the slots, in double and in a fixed order.  No floating-point atomics: two calls give the same bits.
#include "workspace.h"
#include <math.h>

namespace mcr {

constexpr int DH_MAX_C = 512;
constexpr int DH_CC = 8, DH_CC_SMALL = 24;           // channels staged in LDS per pass of the forward: 32 x 8 tile, 16 x 4 tile
constexpr int DH_CG = 4;                             // channels per workgroup of the weight-gradient kernel
constexpr int DH_WT_W = 64, DH_WT_H = 16;            // that kernel's tile: 256 threads, a wave per row, 4 rows a thread
constexpr int DH_WT_ROWS = 4;
constexpr int DH_NSUM = DH_CG * 9 + 1;               // its sums: the 9 DH_CG weight gradients and sum g

__device__ __forceinline__ int dh_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // i in -1 .. n, n >= 2

// grid (tiles B), NT threads of which the first TW TH own a pixel each; all of them stage.  z may be NULL.
template <int TW, int TH, int NT, int CC>
__global__ __launch_bounds__(NT) void dh_forward_kernel(const float* __restrict__ x, const float* __restrict__ weight,
                                                        const float* __restrict__ bias, float* __restrict__ y, float* __restrict__ z, int C,
                                                        int Hs, int Ws, int tiles_x, int tiles) {
    constexpr int RW = TW + 2, R = RW * (TH + 2), K = (CC * R + NT - 1) / NT;
    static_assert(TW * TH <= NT, "a thread per pixel");
    __shared__ float xs[CC * R];
    const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const bool owner = threadIdx.x < TW * TH;
    const int ty = owner ? threadIdx.x / TW : 0, tx = threadIdx.x % TW;
    const int i = y0 + ty, j = x0 + tx;
    const size_t plane = (size_t)Hs * Ws;
    const float* xb = x + (size_t)b * C * plane;
    // A pass of CC channels travels through K registers a thread, all loads in flight at once: element e = c R + ry RW + rx of the pass is the
    // padded coordinate (y0 - 1 + ry, x0 - 1 + rx) of channel c0 + c; a coordinate past n is read by no pixel of the image.
    float v[K];
    auto load = [&](int c0) {
        const int n = min(CC, C - c0) * R;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = threadIdx.x + k * NT;
            const int c = e / R, r = e - c * R;
            const int ry = r / RW, rx = r - ry * RW;
            const int cy = y0 - 1 + ry, cx = x0 - 1 + rx;          // >= -1
            v[k] = e < n && cy <= Hs && cx <= Ws ? xb[(size_t)(c0 + c) * plane + (size_t)dh_reflect(cy, Hs) * Ws + dh_reflect(cx, Ws)] : 0.f;
        }
    };
    float acc = bias[0];
    load(0);
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int nc = min(CC, C - c0);
        __syncthreads();                                           // the pass before this one has been read
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((int)threadIdx.x + k * NT < nc * R) xs[threadIdx.x + k * NT] = v[k];
        __syncthreads();
        if (c0 + CC < C) load(c0 + CC);                            // the next pass is on its way while this one is added
        if (!owner) continue;
        const float* w = weight + (size_t)c0 * 9;                  // wave-uniform: scalar loads
        for (int c = 0; c < nc; ++c) {
            const float* p = xs + c * R + ty * RW + tx;
#pragma unroll
            for (int di = 0; di < 3; ++di)
#pragma unroll
                for (int dj = 0; dj < 3; ++dj) acc = fmaf(w[c * 9 + di * 3 + dj], p[di * RW + dj], acc);
        }
    }
    if (owner && i < Hs && j < Ws) {
        const size_t o = (size_t)b * plane + (size_t)i * Ws + j;
        if (z) z[o] = acc;
        y[o] = 1.f / (1.f + expf(-acc));
    }
}

// g = d_y y (1 - y) of the tile at (y0, x0) and its ring: gs[ry RW + rx] is pixel (y0 - 1 + ry, x0 - 1 + rx), 0 outside the image;
// gs[RW (TH + 2)] = 0, the cell an absent source points to.
template <int TW, int TH>
__device__ __forceinline__ void dh_fill_g(const float* __restrict__ y, const float* __restrict__ d_y, size_t image, int Hs, int Ws, int y0,
                                          int x0, float* gs) {
    constexpr int RW = TW + 2, R = RW * (TH + 2);
    for (int r = threadIdx.x; r <= R; r += blockDim.x) {
        const int ry = r / RW, rx = r - ry * RW;
        const int cy = y0 - 1 + ry, cx = x0 - 1 + rx;
        float v = 0.f;
        if (r < R && cy >= 0 && cy < Hs && cx >= 0 && cx < Ws) {
            const size_t o = image + (size_t)cy * Ws + cx;
            const float yy = y[o];
            v = d_y[o] * yy * (1.f - yy);
        }
        gs[r] = v;
    }
}

// S[t] of pixel (i, j), whose region coordinate is (lr, lc): per axis and tap, the direct source (always a region cell: 0 where it lies
// outside the image) and the mirrored one (-1: none).
template <int RW, int ZERO>
__device__ __forceinline__ void dh_gather(const float* gs, int i, int j, int lr, int lc, int Hs, int Ws, float (&S)[9]) {
    const int ra[3] = {lr + 1, lr, lr - 1}, rb[3] = {i == 1 ? lr - 1 : -1, -1, i == Hs - 2 ? lr + 1 : -1};
    const int ca[3] = {lc + 1, lc, lc - 1}, cb[3] = {j == 1 ? lc - 1 : -1, -1, j == Ws - 2 ? lc + 1 : -1};
#pragma unroll
    for (int di = 0; di < 3; ++di)
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const float aa = gs[ra[di] * RW + ca[dj]];
            const float ab = gs[cb[dj] < 0 ? ZERO : ra[di] * RW + cb[dj]];
            const float ba = gs[rb[di] < 0 ? ZERO : rb[di] * RW + ca[dj]];
            const float bb = gs[rb[di] < 0 || cb[dj] < 0 ? ZERO : rb[di] * RW + cb[dj]];
            S[di * 3 + dj] = (aa + ab) + (ba + bb);
        }
}

// grid (tiles B): d_x[b,c,p] = sum_t weight[c,t] S_t[b,p], a thread per pixel, the channels ascending.
template <int TW, int TH>
__global__ __launch_bounds__(TW* TH) void dh_backward_x_kernel(const float* __restrict__ weight, const float* __restrict__ y,
                                                              const float* __restrict__ d_y, float* __restrict__ d_x, int C, int Hs, int Ws,
                                                              int tiles_x, int tiles) {
    constexpr int RW = TW + 2, R = RW * (TH + 2);
    __shared__ float gs[R + 1];
    const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const size_t plane = (size_t)Hs * Ws;
    dh_fill_g<TW, TH>(y, d_y, (size_t)b * plane, Hs, Ws, y0, x0, gs);
    __syncthreads();
    const int ty = threadIdx.x / TW, tx = threadIdx.x % TW;
    const int i = y0 + ty, j = x0 + tx;
    if (i >= Hs || j >= Ws) return;
    float S[9];
    dh_gather<RW, R>(gs, i, j, ty + 1, tx + 1, Hs, Ws, S);
    float* dst = d_x + (size_t)b * C * plane + (size_t)i * Ws + j;
    for (int c = 0; c < C; ++c) {
        const float* w = weight + c * 9;                           // wave-uniform: scalar loads
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(w[t], S[t], acc);
        dst[(size_t)c * plane] = acc;
    }
}

// grid (tiles B, ceil(C / DH_CG)).  part[o n_parts + n], n = blockIdx.x: output o = c 9 + t, and o = 9 C the bias (channel group 0 stores it).
__global__ __launch_bounds__(256) void dh_backward_w_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ d_y,
                                                            float* __restrict__ part, int C, int Hs, int Ws, int tiles_x, int tiles) {
    constexpr int RW = DH_WT_W + 2, R = RW * (DH_WT_H + 2);
    __shared__ float gs[R + 1], red[4][DH_NSUM];
    const int tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
    const int y0 = (tile / tiles_x) * DH_WT_H, x0 = (tile % tiles_x) * DH_WT_W;
    const int c0 = blockIdx.y * DH_CG;
    const size_t plane = (size_t)Hs * Ws;
    dh_fill_g<DH_WT_W, DH_WT_H>(y, d_y, (size_t)b * plane, Hs, Ws, y0, x0, gs);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // the lane is the column, the wave the row modulo 4
    const int j = x0 + lane;
    float acc[DH_NSUM];
#pragma unroll
    for (int k = 0; k < DH_NSUM; ++k) acc[k] = 0.f;
    for (int k = 0; k < DH_WT_ROWS; ++k) {
        const int ty = wave + 4 * k, i = y0 + ty;
        if (i >= Hs || j >= Ws) continue;
        float S[9];
        dh_gather<RW, R>(gs, i, j, ty + 1, lane + 1, Hs, Ws, S);
        acc[DH_NSUM - 1] += gs[(ty + 1) * RW + lane + 1];
        const float* src = x + ((size_t)b * C + c0) * plane + (size_t)i * Ws + j;
#pragma unroll
        for (int c = 0; c < DH_CG; ++c) {
            if (c0 + c >= C) continue;                             // wave-uniform
            const float xv = src[(size_t)c * plane];
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[c * 9 + t] = fmaf(xv, S[t], acc[c * 9 + t]);
        }
    }
#pragma unroll
    for (int k = 0; k < DH_NSUM; ++k) {
        const float v = wave_sum_all(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < DH_NSUM) {
        const int k = threadIdx.x;
        const float total = four_wave_sum(&red[0][k], DH_NSUM);
        const size_t n_parts = gridDim.x;
        if (k < DH_NSUM - 1) {
            const int c = c0 + k / 9;
            if (c < C) part[((size_t)c * 9 + k % 9) * n_parts + blockIdx.x] = total;
        } else if (blockIdx.y == 0) {
            part[(size_t)C * 9 * n_parts + blockIdx.x] = total;
        }
    }
}

// grid (ceil((9 C + 1) / 4)): a wave per output adds its n_parts partials, lane l the slots l, l + 64, .. ascending, in double.
__global__ __launch_bounds__(256) void dh_backward_finish_kernel(const float* __restrict__ part, float* __restrict__ d_weight,
                                                                 float* __restrict__ d_bias, int C, int64_t n_parts) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o > C * 9) return;
    const float* p = part + (size_t)o * n_parts;
    double acc = 0.0;
    for (int64_t n = lane; n < n_parts; n += 64) acc += (double)p[n];
    acc = wave_sum_all(acc);
    if (lane != 0) return;
    if (o < C * 9) {
        if (d_weight) d_weight[o] = (float)acc;
    } else if (d_bias) {
        d_bias[0] = (float)acc;
    }
}

// The tile of the forward and of the d_x gather: 32 x 8, or 16 x 4 where that gives fewer workgroups than the 256 compute units.
static bool dh_small_tile(int64_t B, int64_t Hs, int64_t Ws) { return B * cdiv(Hs, 8) * cdiv(Ws, 32) < 256; }

static bool dh_sizes_ok(int64_t B, int64_t C, int64_t Hs, int64_t Ws) {
    if (B < 1 || C < 1 || C > DH_MAX_C || Hs < 2 || Ws < 2) return false;
    if (Hs > 0x7fffffffll || Ws > 0x7fffffffll || Hs * Ws > 0x7fffffffll) return false;
    return B <= 0x7fffffffll / (C * Hs * Ws);                      // B C Hs Ws, the largest operand, fits a 32-bit index
}

struct DhBwdScratch { float* part; };                 // [9 C + 1, B tiles] of the 64 x 16 tiles
static DhBwdScratch carve_dh_bwd(Arena& a, int64_t B, int64_t C, int64_t Hs, int64_t Ws) {
    DhBwdScratch w;
    w.part = a.f((size_t)(9 * C + 1) * (size_t)(B * cdiv(Hs, DH_WT_H) * cdiv(Ws, DH_WT_W)));
    return w;
}

static int dh_check(const char* who, int64_t B, int C, int Hs, int Ws) {
    MCR_REQUIRE(Hs >= 2 && Ws >= 2, "%s: the map is %d x %d, Hs and Ws must be at least 2 (the reflection padding)", who, Hs, Ws);
    MCR_REQUIRE(C >= 1 && C <= DH_MAX_C, "%s: C = %d channels, 1 .. %d are supported", who, C, DH_MAX_C);
    MCR_REQUIRE(B >= 1, "%s: B = %lld must be at least 1", who, (long long)B);
    MCR_REQUIRE(dh_sizes_ok(B, C, Hs, Ws), "%s: B = %lld, C = %d, %d x %d: a product of the sizes overflows a 32-bit index", who, (long long)B, C,
                Hs, Ws);
    return 0;
}

}  // namespace mcr

using namespace mcr;

extern "C" int mcr_disparity_head(const float* x, const float* weight, const float* bias, float* y, float* z, int64_t B, int C, int Hs, int Ws,
                                  void* stream) {
    const char* who = "mcr_disparity_head";
    if (int e = dh_check(who, B, C, Hs, Ws)) return e;
    MCR_REQUIRE(x && weight && bias && y, "%s: NULL operand", who);
    const hipStream_t st = (hipStream_t)stream;
    if (dh_small_tile(B, Hs, Ws)) {
        const int tx = (int)cdiv(Ws, 16), tiles = tx * (int)cdiv(Hs, 4);
        hipLaunchKernelGGL((dh_forward_kernel<16, 4, 256, DH_CC_SMALL>), dim3((unsigned)(tiles * B)), dim3(256), 0, st, x, weight, bias, y, z, C, Hs, Ws, tx, tiles);
    } else {
        const int tx = (int)cdiv(Ws, 32), tiles = tx * (int)cdiv(Hs, 8);
        hipLaunchKernelGGL((dh_forward_kernel<32, 8, 256, DH_CC>), dim3((unsigned)(tiles * B)), dim3(256), 0, st, x, weight, bias, y, z, C, Hs, Ws, tx, tiles);
    }
    MCR_LAUNCH_CHECK("dh_forward_kernel");
    return 0;
}

extern "C" size_t mcr_disparity_head_backward_workspace_bytes(int64_t B, int64_t C, int64_t Hs, int64_t Ws) {
    if (!dh_sizes_ok(B, C, Hs, Ws)) return 0;
    return measure(carve_dh_bwd, B, C, Hs, Ws);
}

extern "C" int mcr_disparity_head_backward(const float* x, const float* weight, const float* y, const float* d_y, float* d_x, float* d_weight,
                                           float* d_bias, int64_t B, int C, int Hs, int Ws, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    const char* who = "mcr_disparity_head_backward";
    if (int e = dh_check(who, B, C, Hs, Ws)) return e;
    MCR_REQUIRE(d_x || d_weight || d_bias, "%s: d_x, d_weight and d_bias are all NULL, nothing to do", who);
    MCR_REQUIRE(y && d_y && (!d_x || weight) && (!d_weight || x), "%s: NULL operand", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_disparity_head_backward_workspace_bytes(B, C, Hs, Ws))) return e;
    const hipStream_t st = (hipStream_t)stream;
    if (d_x) {
        if (dh_small_tile(B, Hs, Ws)) {
            const int tx = (int)cdiv(Ws, 16), tiles = tx * (int)cdiv(Hs, 4);
            hipLaunchKernelGGL((dh_backward_x_kernel<16, 4>), dim3((unsigned)(tiles * B)), dim3(64), 0, st, weight, y, d_y, d_x, C, Hs, Ws, tx, tiles);
        } else {
            const int tx = (int)cdiv(Ws, 32), tiles = tx * (int)cdiv(Hs, 8);
            hipLaunchKernelGGL((dh_backward_x_kernel<32, 8>), dim3((unsigned)(tiles * B)), dim3(256), 0, st, weight, y, d_y, d_x, C, Hs, Ws, tx, tiles);
        }
        MCR_LAUNCH_CHECK("dh_backward_x_kernel");
    }
    if (d_weight || d_bias) {
        Arena arena{(char*)workspace, workspace_bytes};
        const DhBwdScratch ws = carve_dh_bwd(arena, B, C, Hs, Ws);
        const int tx = (int)cdiv(Ws, DH_WT_W), tiles = tx * (int)cdiv(Hs, DH_WT_H);
        const int64_t n_parts = (int64_t)tiles * B;
        // without d_weight only channel group 0 runs: it alone stores the bias partials (x may then be NULL: it is read at c < C_eff = 0)
        const int C_eff = d_weight ? C : 0;
        hipLaunchKernelGGL(dh_backward_w_kernel, dim3((unsigned)n_parts, (unsigned)(d_weight ? cdiv(C, DH_CG) : 1)), dim3(256), 0, st, x, y, d_y,
                           ws.part + (d_weight ? 0 : (size_t)9 * C * n_parts), C_eff, Hs, Ws, tx, tiles);
        MCR_LAUNCH_CHECK("dh_backward_w_kernel");
        if (d_weight) {
            hipLaunchKernelGGL(dh_backward_finish_kernel, dim3((unsigned)cdiv(9 * C + 1, 4)), dim3(256), 0, st, ws.part, d_weight, d_bias, C, n_parts);
        } else {
            hipLaunchKernelGGL(dh_backward_finish_kernel, dim3(1), dim3(256), 0, st, ws.part + (size_t)9 * C * n_parts, (float*)nullptr, d_bias, 0,
                               n_parts);
        }
        MCR_LAUNCH_CHECK("dh_backward_finish_kernel");
    }
    return 0;
}
