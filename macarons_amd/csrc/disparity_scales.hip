// What a depth-training step does between the depth network's disparity maps and its two losses (macarons/utility/macarons_utils.py:959-1031
// apply_depth_model, with get_regularity_loss_fn / regularity_tab of depth_model_utils.py:522-562), fused, for gfx950 -- forward and backward:
// the disparity-to-depth conversions, the nearest upsamplings, the per-image mean normalisations, the mask zeroing, the edge-aware
// regularity value of every scale and the error mask of scale 0.
//
// Per scale s (disp_s [B,H_s,W_s], H = r_s H_s, W = r_s W_s, r_s a power of two up to 16), image b and full-resolution pixel p = (y, x):
//   D[p]     = disp_s[b, y / r_s, x / r_s]            (read directly: upstream's depth -> disparity round trip is the identity to 6e-8)
//   depth[p] = 1 / (a D[p] + b0),  a = 1/znear - 1/zfar, b0 = 1/zfar
//   n[p]     = mask[p] ? D[p] / (mu + 1e-7) : 0,  mu the mean of D over the image (= the mean of disp_s[b]: every value is repeated r_s^2 times)
//   e_x[p]   = exp(-mean_c |I[y,x] - I[y,x+1]|),  e_y[p] = exp(-mean_c |I[y,x] - I[y+1,x]|)         (once for all scales)
//   reg[s]   = mean over B H (W-1) of |n[y,x] - n[y,x+1]| e_x  +  mean over B (H-1) W of |n[y,x] - n[y+1,x]| e_y
// and, from scale 0 alone, with P(i,j) = n[rho(i), rho(j)], rho(i) = reflect(i - 1) (upstream's table on reflection-padded copies, with its
// one-pixel shift up and left):
//   tab[i,j] = |P(i,j) - P(i,j+1)| exp(-mean_c |I_P(i,j) - I_P(i,j+1)|) + |P(i,j) - P(i+1,j)| exp(-mean_c |I_P(i,j) - I_P(i+1,j)|)
//   thr[b]   = mean(tab_b) + std(tab_b) (unbiased),  error_mask = tab < thr
//
// Forward, four launches: ds_mean_kernel (the S B sums, at each scale's own resolution, DS_CHUNKS double partials an image);
// ds_forward_kernel (a workgroup owns a 16 x 16 tile of one image for ALL scales: it holds the image and the S normalised disparities of the
// tile and a one-pixel ring in LDS, the ring reflected at the top and left border as the table needs it, writes the depths and the table,
// and stores one partial per regularity sum and the tile's sum and sum of squares of the table, in double); ds_finish_kernel (one workgroup
// adds the partials in a fixed order, in double: the variance is (sum t^2 - (sum t)^2 / N) / (N - 1) of exact double squares of fp32 values,
// never an fp32 E[t^2] - mean^2); ds_mask_kernel (tab < thr).  No floating-point atomics.
//
// Backward, three launches with d_reg, one without: ds_mean_kernel; ds_backward_kernel (the same tile: per pixel
//   local[p] = -a depth[p]^2 d_depth[s,b,p] + m[p] G[p] / (mu + eps),   G = d_reg[s] d reg[s] / d n[p]  (sign(0) = 0),
// summed per r_s x r_s block in a fixed order from LDS -- a block never straddles a tile, 16 is a multiple of every ratio -- and written to
// d_disp_s, plus the tile's partial of sum m G D); ds_backward_mean_kernel (adds an image's partials in a fixed order and subtracts
// sum m G D / ((mu + eps)^2 H_s W_s), the derivative through the mean, from every pixel of d_disp_s[b]).  Both directions form n with the
// same operations from the same partials, so they agree on every sign bit for bit.
#include "workspace.h"
#include <math.h>

namespace mcr {

constexpr int DS_T = 16;                             // tile edge: 256 threads, one pixel each; a multiple of every ratio
constexpr int DS_MAX_S = 8;                          // scales
constexpr int DS_MAX_SHIFT = 4;                      // ratios 1, 2, 4, 8, 16
constexpr int DS_CHUNKS = 32;                        // workgroups that sum one image of one scale
constexpr int DS_RW = DS_T + 2, DS_R = DS_RW * DS_RW;   // the tile and its ring in LDS

struct DsArgs {
    const float* disp[DS_MAX_S];                     // [B,H_s,W_s]
    float* d_disp[DS_MAX_S];                         // [B,H_s,W_s] (backward)
    int shift[DS_MAX_S];                             // log2 r_s
    const float* images;                             // [B,H,W,3]
    const unsigned char* mask;                       // [B,H,W] or NULL
    int S, B, H, W, tiles_x;
    float a, b0;
};

// The by-value argument struct is indexed with compile-time constants only (a run-time index would copy it to scratch).
#define DS_FOR_SCALES(s) _Pragma("unroll") for (int s = 0; s < DS_MAX_S; ++s) if (s < g.S)

// part[((s B) + b) DS_CHUNKS + c] = the sum of chunk c of disp_s[b], in double.  grid (DS_CHUNKS, B, S).
__global__ __launch_bounds__(256) void ds_mean_kernel(DsArgs g, double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.x, b = blockIdx.y, sc = blockIdx.z;
    const float* src = nullptr;
    int sh = 0;
    DS_FOR_SCALES(s) if (s == sc) src = g.disp[s], sh = g.shift[s];
    const int64_t n = (int64_t)(g.H >> sh) * (g.W >> sh);
    src += (size_t)b * n;
    int64_t i0, i1;
    chunk_range(n, DS_CHUNKS, c, i0, i1);
    double acc = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc += (double)src[i];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[((size_t)sc * g.B + b) * DS_CHUNKS + c] = acc;
}

// den[s] = mu_{s,b} + 1e-7 in fp32, from the chunk sums in ascending order: thread s of the workgroup.
__device__ __forceinline__ void ds_means(const DsArgs& g, const double* __restrict__ mean_part, int b, float* den) {
    DS_FOR_SCALES(s) if ((int)threadIdx.x == s) {
        const double* pp = mean_part + ((size_t)s * g.B + b) * DS_CHUNKS;
        double acc = 0.0;
        for (int c = 0; c < DS_CHUNKS; ++c) acc += pp[c];
        const double n = (double)(g.H >> g.shift[s]) * (double)(g.W >> g.shift[s]);
        den[s] = (float)(acc / n) + 1e-7f;
    }
}

__device__ __forceinline__ float ds_disp_at(const DsArgs& g, const float* __restrict__ src, int sh, int b, int p, int q) {
    const int Hs = g.H >> sh, Ws = g.W >> sh;
    return src[((size_t)b * Hs + (p >> sh)) * Ws + (q >> sh)];
}

// The tile at (y0, x0) and its ring: region index r = ry DS_RW + rx is the padded coordinate (y0 - 1 + ry, x0 - 1 + rx); coordinate -1 is
// pixel 1 (the table's reflection), a coordinate past the last row or column belongs to no pair and holds 0.
// img[c DS_R + r] the image, nrm[s DS_R + r] the normalised disparity n of scale s.
__device__ __forceinline__ void ds_fill(const DsArgs& g, int b, int y0, int x0, const float* den, float* img, float* nrm) {
    const int H = g.H, W = g.W;
    for (int r = threadIdx.x; r < DS_R; r += DS_T * DS_T) {
        const int ry = r / DS_RW, rx = r - ry * DS_RW;
        const int cy = y0 - 1 + ry, cx = x0 - 1 + rx;              // >= -1
        if (cy >= H || cx >= W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) img[c * DS_R + r] = 0.f;
            DS_FOR_SCALES(s) nrm[s * DS_R + r] = 0.f;
            continue;
        }
        const int p = cy < 0 ? 1 : cy, q = cx < 0 ? 1 : cx;        // H, W >= 2
        const size_t pix = ((size_t)b * H + p) * W + q;
#pragma unroll
        for (int c = 0; c < 3; ++c) img[c * DS_R + r] = g.images[pix * 3 + c];
        const bool on = !g.mask || g.mask[pix];
        DS_FOR_SCALES(s) {
            const float D = ds_disp_at(g, g.disp[s], g.shift[s], b, p, q);
            nrm[s * DS_R + r] = on ? D / den[s] : 0.f;             // zeroed by selection
        }
    }
}

// exp(-mean_c |I[i] - I[j]|) of two region indices.
__device__ __forceinline__ float ds_weight(const float* img, int i, int j) {
    const float d = (fabsf(img[i] - img[j]) + fabsf(img[DS_R + i] - img[DS_R + j])) + fabsf(img[2 * DS_R + i] - img[2 * DS_R + j]);
    return expf(-(d / 3.f));
}

__device__ __forceinline__ float ds_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// grid (tiles, B).  part_reg[(b tiles + tile) 2S + k]: k < S the x sums, then the y sums; part_tab[(b tiles + tile) 2 + {0, 1}]: sum t, sum t^2.
__global__ __launch_bounds__(DS_T* DS_T) void ds_forward_kernel(DsArgs g, const double* __restrict__ mean_part, float* __restrict__ depth,
                                                               float* __restrict__ tab, float* __restrict__ part_reg,
                                                               double* __restrict__ part_tab) {
    __shared__ float img[3 * DS_R], nrm[DS_MAX_S * DS_R], den[DS_MAX_S], redf[4][2 * DS_MAX_S];
    __shared__ double redd[4][2];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int y0 = (tile / g.tiles_x) * DS_T, x0 = (tile % g.tiles_x) * DS_T;
    const int H = g.H, W = g.W;
    ds_means(g, mean_part, b, den);
    __syncthreads();
    ds_fill(g, b, y0, x0, den, img, nrm);
    __syncthreads();
    const int ty = threadIdx.x / DS_T, tx = threadIdx.x % DS_T;
    const int p = y0 + ty, q = x0 + tx;
    float sx[DS_MAX_S], sy[DS_MAX_S];
#pragma unroll
    for (int s = 0; s < DS_MAX_S; ++s) sx[s] = sy[s] = 0.f;
    double t1 = 0.0, t2 = 0.0;
    if (p < H && q < W) {
        const int rc = (ty + 1) * DS_RW + tx + 1;
        const size_t pix = ((size_t)b * H + p) * W + q;
        DS_FOR_SCALES(s) {
            const float D = ds_disp_at(g, g.disp[s], g.shift[s], b, p, q);
            depth[(size_t)s * g.B * H * W + pix] = 1.f / (g.a * D + g.b0);
        }
        const bool hasx = q + 1 < W, hasy = p + 1 < H;
        const float ex = hasx ? ds_weight(img, rc, rc + 1) : 0.f, ey = hasy ? ds_weight(img, rc, rc + DS_RW) : 0.f;
        DS_FOR_SCALES(s) {
            const float n0 = nrm[s * DS_R + rc];
            sx[s] = hasx ? fabsf(n0 - nrm[s * DS_R + rc + 1]) * ex : 0.f;
            sy[s] = hasy ? fabsf(n0 - nrm[s * DS_R + rc + DS_RW]) * ey : 0.f;
        }
        // the table of scale 0: P(i,j) sits one up and one left in the region (padded coordinate (p - 1, q - 1), reflected by the fill)
        const int pc = rc - DS_RW - 1;
        const float tx_ = fabsf(nrm[pc] - nrm[pc + 1]) * ds_weight(img, pc, pc + 1);
        const float ty_ = fabsf(nrm[pc] - nrm[pc + DS_RW]) * ds_weight(img, pc, pc + DS_RW);
        const float t = tx_ + ty_;
        tab[pix] = t;
        t1 = (double)t, t2 = (double)t * (double)t;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    DS_FOR_SCALES(s) {
        const float vx = wave_sum_all(sx[s]), vy = wave_sum_all(sy[s]);
        if (lane == 0) redf[wave][s] = vx, redf[wave][g.S + s] = vy;
    }
    t1 = wave_sum_all(t1), t2 = wave_sum_all(t2);
    if (lane == 0) redd[wave][0] = t1, redd[wave][1] = t2;
    __syncthreads();
    const size_t slot = (size_t)b * gridDim.x + tile;
    if ((int)threadIdx.x < 2 * g.S) {
        const int k = threadIdx.x;
        part_reg[slot * 2 * g.S + k] = four_wave_sum(&redf[0][k], 2 * DS_MAX_S);
    }
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part_tab[slot * 2 + k] = four_wave_sum(&redd[0][k], 2);
    }
}

// One workgroup: a wave per sum adds that sum's tile partials in a fixed order, in double; then a thread per scale forms reg[s] (the
// images ascending) and a thread per image thr[b].  sb: 2 S B + 2 B doubles.
__global__ __launch_bounds__(256) void ds_finish_kernel(const float* __restrict__ part_reg, const double* __restrict__ part_tab,
                                                        double* __restrict__ sb, float* __restrict__ reg, float* __restrict__ thr, int S, int B,
                                                        int H, int W, int n_tiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_reg = (int64_t)B * 2 * S;
    for (int64_t i = wave; i < n_reg + 2 * (int64_t)B; i += 4) {
        double acc = 0.0;
        if (i < n_reg) {
            const int64_t b = i / (2 * S), k = i - b * 2 * S;
            for (int t = lane; t < n_tiles; t += 64) acc += (double)part_reg[(b * n_tiles + t) * 2 * S + k];
        } else {
            const int64_t j = i - n_reg, b = j >> 1, k = j & 1;
            for (int t = lane; t < n_tiles; t += 64) acc += part_tab[(b * n_tiles + t) * 2 + k];
        }
        acc = wave_sum_all(acc);
        if (lane == 0) sb[i] = acc;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += 256) {
        double x = 0.0, y = 0.0;
        for (int b = 0; b < B; ++b) x += sb[(int64_t)b * 2 * S + s], y += sb[(int64_t)b * 2 * S + S + s];
        reg[s] = (float)(x / ((double)B * H * (W - 1)) + y / ((double)B * (H - 1) * W));
    }
    for (int b = threadIdx.x; b < B; b += 256) {
        const double N = (double)H * W, s1 = sb[n_reg + 2 * (int64_t)b], s2 = sb[n_reg + 2 * (int64_t)b + 1];
        const double mean = s1 / N, var = fmax((s2 - s1 * mean) / (N - 1.0), 0.0);        // N >= 4
        thr[b] = (float)(mean + sqrt(var));
    }
}

// error_mask = tab < thr[b].  grid (ceil(H W / 256), B).
__global__ __launch_bounds__(256) void ds_mask_kernel(const float* __restrict__ tab, const float* __restrict__ thr, unsigned char* __restrict__ em,
                                                      int64_t n_pix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    const size_t o = (size_t)blockIdx.y * n_pix + i;
    em[o] = tab[o] < thr[blockIdx.y] ? 1 : 0;
}

// grid (tiles, B).  Writes the block sums of the local terms to d_disp_s; with d_reg also part[(b tiles + tile) S + s] = sum m G D.
__global__ __launch_bounds__(DS_T* DS_T) void ds_backward_kernel(DsArgs g, const double* __restrict__ mean_part, const float* __restrict__ d_depth,
                                                                const float* __restrict__ d_reg, double* __restrict__ part) {
    __shared__ float img[3 * DS_R], nrm[DS_MAX_S * DS_R], den[DS_MAX_S], val[DS_MAX_S * DS_T * DS_T];
    __shared__ double redd[4][DS_MAX_S];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int y0 = (tile / g.tiles_x) * DS_T, x0 = (tile % g.tiles_x) * DS_T;
    const int H = g.H, W = g.W;
    if (d_reg) {
        ds_means(g, mean_part, b, den);
        __syncthreads();
        ds_fill(g, b, y0, x0, den, img, nrm);
        __syncthreads();
    }
    const int ty = threadIdx.x / DS_T, tx = threadIdx.x % DS_T;
    const int p = y0 + ty, q = x0 + tx;
    const bool in = p < H && q < W;
    double mgd[DS_MAX_S];
#pragma unroll
    for (int s = 0; s < DS_MAX_S; ++s) mgd[s] = 0.0;
    DS_FOR_SCALES(s) val[s * DS_T * DS_T + threadIdx.x] = 0.f;
    if (in) {
        const int rc = (ty + 1) * DS_RW + tx + 1;
        const size_t pix = ((size_t)b * H + p) * W + q;
        const bool on = !g.mask || g.mask[pix];
        // the four pairs this pixel belongs to, with the pair's weight over the size of its mean; a pair outside the image has weight 0
        float wr = 0.f, wl = 0.f, wd = 0.f, wu = 0.f;
        if (d_reg && on) {
            const float cx = (float)(1.0 / ((double)g.B * H * (W - 1))), cy = (float)(1.0 / ((double)g.B * (H - 1) * W));
            wr = q + 1 < W ? cx * ds_weight(img, rc, rc + 1) : 0.f;
            wl = q > 0 ? cx * ds_weight(img, rc - 1, rc) : 0.f;
            wd = p + 1 < H ? cy * ds_weight(img, rc, rc + DS_RW) : 0.f;
            wu = p > 0 ? cy * ds_weight(img, rc - DS_RW, rc) : 0.f;
        }
        DS_FOR_SCALES(s) {
            const float D = ds_disp_at(g, g.disp[s], g.shift[s], b, p, q);
            float local = 0.f;
            if (d_depth) {
                const float dep = 1.f / (g.a * D + g.b0);
                local = -g.a * dep * dep * d_depth[(size_t)s * g.B * H * W + pix];
            }
            if (d_reg && on) {
                const float* ns = nrm + s * DS_R;
                const float n0 = ns[rc];
                // a neighbour's region entry is read only where its weight is not 0 (q > 0, p > 0: no reflected entry enters)
                const float gx = (q + 1 < W ? ds_sign(n0 - ns[rc + 1]) * wr : 0.f) - (q > 0 ? ds_sign(ns[rc - 1] - n0) * wl : 0.f);
                const float gy = (p + 1 < H ? ds_sign(n0 - ns[rc + DS_RW]) * wd : 0.f) - (p > 0 ? ds_sign(ns[rc - DS_RW] - n0) * wu : 0.f);
                const float G = d_reg[s] * (gx + gy);
                local += G / den[s];
                mgd[s] = (double)G * (double)D;
            }
            val[s * DS_T * DS_T + threadIdx.x] = local;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (d_reg) {
        DS_FOR_SCALES(s) {
            const double v = wave_sum_all(mgd[s]);
            if (lane == 0) redd[wave][s] = v;
        }
    }
    __syncthreads();
    if (d_reg && (int)threadIdx.x < g.S) {
        const int s = threadIdx.x;
        part[((size_t)b * gridDim.x + tile) * g.S + s] = four_wave_sum(&redd[0][s], DS_MAX_S);
    }
    // the r x r blocks of the tile, each summed row-major by one thread
    DS_FOR_SCALES(s) {
        const int sh = g.shift[s], r = 1 << sh, nb = DS_T >> sh;
        const int Hs = H >> sh, Ws = W >> sh;
        for (int t = threadIdx.x; t < nb * nb; t += DS_T * DS_T) {
            const int by = t / nb, bx = t - by * nb;
            const int P = (y0 >> sh) + by, Q = (x0 >> sh) + bx;
            if (P >= Hs || Q >= Ws) continue;                       // H = r H_s: a block lies wholly inside the image or wholly outside
            const float* v = val + s * DS_T * DS_T + (by * r) * DS_T + bx * r;
            float acc = 0.f;
            for (int yy = 0; yy < r; ++yy)
                for (int xx = 0; xx < r; ++xx) acc += v[yy * DS_T + xx];
            g.d_disp[s][((size_t)b * Hs + P) * Ws + Q] = acc;
        }
    }
}

// grid (DS_CHUNKS, B, S): d_disp_s[b] -= sum over the tiles of part / ((mu + eps)^2 H_s W_s); every workgroup of an image adds the same
// partials in the same order.
__global__ __launch_bounds__(256) void ds_backward_mean_kernel(DsArgs g, const double* __restrict__ mean_part, const double* __restrict__ part,
                                                               int n_tiles) {
    __shared__ double red[4];
    __shared__ float den[DS_MAX_S];
    const int c = blockIdx.x, b = blockIdx.y, sc = blockIdx.z;
    ds_means(g, mean_part, b, den);
    double acc = 0.0;
    for (int t = threadIdx.x; t < n_tiles; t += 256) acc += part[((size_t)b * n_tiles + t) * g.S + sc];
    acc = block_sum_256(acc, red);
    float* dst = nullptr;
    int sh = 0;
    DS_FOR_SCALES(s) if (s == sc) dst = g.d_disp[s], sh = g.shift[s];
    const int64_t n = (int64_t)(g.H >> sh) * (g.W >> sh);
    const double dn = (double)den[sc];
    const float sub = (float)(acc / (dn * dn * (double)n));
    dst += (size_t)b * n;
    int64_t i0, i1;
    chunk_range(n, DS_CHUNKS, c, i0, i1);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) dst[i] -= sub;
}

static bool ds_sizes_ok(int64_t S, int64_t B, int64_t H, int64_t W) {
    if (S < 1 || S > DS_MAX_S || B < 1 || B > 65535 || H < 2 || W < 2) return false;
    if (H > 0x3fffffffll || W > 0x3fffffffll || H * W > 0x7fffffffll - 4 * DS_T * DS_T) return false;     // int pixel indices, grid x
    if ((double)B * (double)cdiv(H, DS_T) * (double)cdiv(W, DS_T) * 2.0 * (double)S > 2147483647.0) return false;   // the partials
    if ((double)S * (double)B * (double)H * (double)W * 12.0 > 9.0e18) return false;                      // byte offsets
    return true;
}

// The forward's workspace.  tab and thr are the caller's outputs when it asks for them; the scratch copies are carved either way.
struct DsFwdScratch {
    double* mean_part;                               // [S,B,DS_CHUNKS]
    float* part_reg;                                 // [B,tiles,2S]
    double *part_tab, *sb;                           // [B,tiles,2]; 2 S B + 2 B sums
    float *tab, *thr;                                // [B,H,W]; [B]
};
static DsFwdScratch carve_ds_fwd(Arena& a, int64_t S, int64_t B, int64_t H, int64_t W) {
    const size_t tiles = (size_t)(cdiv(H, DS_T) * cdiv(W, DS_T));
    DsFwdScratch w;
    w.mean_part = (double*)a.bytes((size_t)S * B * DS_CHUNKS * sizeof(double));
    w.part_reg = a.f((size_t)B * tiles * 2 * S);
    w.part_tab = (double*)a.bytes((size_t)B * tiles * 2 * sizeof(double));
    w.sb = (double*)a.bytes(((size_t)B * 2 * S + 2 * (size_t)B) * sizeof(double));
    w.tab = a.f((size_t)B * H * W);
    w.thr = a.f((size_t)B);
    return w;
}

struct DsBwdScratch { double *mean_part, *part; };   // [S,B,DS_CHUNKS]; [B,tiles,S]
static DsBwdScratch carve_ds_bwd(Arena& a, int64_t S, int64_t B, int64_t H, int64_t W) {
    const size_t tiles = (size_t)(cdiv(H, DS_T) * cdiv(W, DS_T));
    DsBwdScratch w;
    w.mean_part = (double*)a.bytes((size_t)S * B * DS_CHUNKS * sizeof(double));
    w.part = (double*)a.bytes((size_t)B * tiles * S * sizeof(double));
    return w;
}

// The checks both entries share, and the argument struct (d_disps may be NULL: the forward).
static int ds_prepare(const char* who, const float* const* disps, float* const* d_disps, const int* Hs, const int* Ws, const float* images,
                      const unsigned char* mask, int S, int64_t B, int H, int W, float znear, float zfar, DsArgs& g) {
    MCR_REQUIRE(S >= 1 && S <= DS_MAX_S, "%s: S = %d scales, 1 .. %d are supported", who, S, DS_MAX_S);
    MCR_REQUIRE(disps && Hs && Ws && images, "%s: NULL operand", who);
    MCR_REQUIRE(H >= 2 && W >= 2, "%s: the image is %d x %d, H and W must be at least 2 (the reflection padding)", who, H, W);
    MCR_REQUIRE(B >= 1, "%s: B = %lld must be at least 1", who, (long long)B);
    MCR_REQUIRE(ds_sizes_ok(S, B, H, W), "%s: S = %d, B = %lld, %d x %d: a product of the sizes overflows an index", who, S, (long long)B, H, W);
    MCR_REQUIRE(znear > 0.f && zfar > 0.f && fabsf(znear) < INFINITY && fabsf(zfar) < INFINITY, "%s: znear and zfar must be positive and finite",
                who);
    g.images = images, g.mask = mask;
    g.S = S, g.B = (int)B, g.H = H, g.W = W, g.tiles_x = (int)cdiv(W, DS_T);
    g.a = 1.f / znear - 1.f / zfar, g.b0 = 1.f / zfar;
    for (int s = 0; s < DS_MAX_S; ++s) g.disp[s] = nullptr, g.d_disp[s] = nullptr, g.shift[s] = 0;
    for (int s = 0; s < S; ++s) {
        MCR_REQUIRE(disps[s] && (!d_disps || d_disps[s]), "%s: NULL map of scale %d", who, s);
        MCR_REQUIRE(Hs[s] >= 1 && Ws[s] >= 1, "%s: scale %d is %d x %d", who, s, Hs[s], Ws[s]);
        int sh = -1;
        for (int k = 0; k <= DS_MAX_SHIFT; ++k)
            if ((int64_t)Hs[s] << k == H) sh = k;
        MCR_REQUIRE(sh >= 0, "%s: scale %d has %d rows for an image of %d: the ratio must be 1, 2, 4, 8 or 16", who, s, Hs[s], H);
        MCR_REQUIRE((int64_t)Ws[s] << sh == W, "%s: scale %d is %d x %d for an image of %d x %d: one ratio on both axes, W_s * %d = W", who, s,
                    Hs[s], Ws[s], H, W, 1 << sh);
        g.disp[s] = disps[s], g.d_disp[s] = d_disps ? d_disps[s] : nullptr, g.shift[s] = sh;
    }
    return 0;
}

}  // namespace mcr

using namespace mcr;

extern "C" size_t mcr_disparity_scales_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t W) {
    if (!ds_sizes_ok(S, B, H, W)) return 0;
    return measure(carve_ds_fwd, S, B, H, W);
}

extern "C" int mcr_disparity_scales(const float* const* disps, const int* Hs, const int* Ws, const float* images, const unsigned char* mask,
                                    float* depth, float* reg, unsigned char* error_mask, float* tab, float* thr, int S, int64_t B, int H, int W,
                                    float znear, float zfar, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_disparity_scales";
    DsArgs g;
    if (int e = ds_prepare(who, disps, nullptr, Hs, Ws, images, mask, S, B, H, W, znear, zfar, g)) return e;
    MCR_REQUIRE(depth && reg && error_mask, "%s: NULL depth, reg or error_mask", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_disparity_scales_workspace_bytes(S, B, H, W))) return e;

    const hipStream_t st = (hipStream_t)stream;
    Arena arena{(char*)workspace, workspace_bytes};
    const DsFwdScratch ws = carve_ds_fwd(arena, S, B, H, W);
    float* tab_out = tab ? tab : ws.tab;
    float* thr_out = thr ? thr : ws.thr;
    const int n_tiles = (int)(cdiv(H, DS_T) * cdiv(W, DS_T));
    hipLaunchKernelGGL(ds_mean_kernel, dim3(DS_CHUNKS, (unsigned)B, (unsigned)S), dim3(256), 0, st, g, ws.mean_part);
    MCR_LAUNCH_CHECK("ds_mean_kernel");
    hipLaunchKernelGGL(ds_forward_kernel, dim3((unsigned)n_tiles, (unsigned)B), dim3(DS_T * DS_T), 0, st, g, ws.mean_part, depth, tab_out, ws.part_reg,
                       ws.part_tab);
    MCR_LAUNCH_CHECK("ds_forward_kernel");
    hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(256), 0, st, ws.part_reg, ws.part_tab, ws.sb, reg, thr_out, S, (int)B, H, W, n_tiles);
    MCR_LAUNCH_CHECK("ds_finish_kernel");
    const int64_t n_pix = (int64_t)H * W;
    hipLaunchKernelGGL(ds_mask_kernel, dim3((unsigned)cdiv(n_pix, 256), (unsigned)B), dim3(256), 0, st, tab_out, thr_out, error_mask, n_pix);
    MCR_LAUNCH_CHECK("ds_mask_kernel");
    return 0;
}

extern "C" size_t mcr_disparity_scales_backward_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t W) {
    if (!ds_sizes_ok(S, B, H, W)) return 0;
    return measure(carve_ds_bwd, S, B, H, W);
}

extern "C" int mcr_disparity_scales_backward(const float* const* disps, const int* Hs, const int* Ws, const float* images,
                                             const unsigned char* mask, const float* d_depth, const float* d_reg, float* const* d_disps, int S,
                                             int64_t B, int H, int W, float znear, float zfar, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    const char* who = "mcr_disparity_scales_backward";
    MCR_REQUIRE(d_disps, "%s: NULL d_disps", who);
    DsArgs g;
    if (int e = ds_prepare(who, disps, d_disps, Hs, Ws, images, mask, S, B, H, W, znear, zfar, g)) return e;
    MCR_REQUIRE(d_depth || d_reg, "%s: d_depth and d_reg are both NULL, nothing to do", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_disparity_scales_backward_workspace_bytes(S, B, H, W))) return e;

    const hipStream_t st = (hipStream_t)stream;
    Arena arena{(char*)workspace, workspace_bytes};
    const DsBwdScratch ws = carve_ds_bwd(arena, S, B, H, W);
    const int n_tiles = (int)(cdiv(H, DS_T) * cdiv(W, DS_T));
    if (d_reg) {
        hipLaunchKernelGGL(ds_mean_kernel, dim3(DS_CHUNKS, (unsigned)B, (unsigned)S), dim3(256), 0, st, g, ws.mean_part);
        MCR_LAUNCH_CHECK("ds_mean_kernel");
    }
    hipLaunchKernelGGL(ds_backward_kernel, dim3((unsigned)n_tiles, (unsigned)B), dim3(DS_T * DS_T), 0, st, g, ws.mean_part, d_depth, d_reg, ws.part);
    MCR_LAUNCH_CHECK("ds_backward_kernel");
    if (d_reg) {
        hipLaunchKernelGGL(ds_backward_mean_kernel, dim3(DS_CHUNKS, (unsigned)B, (unsigned)S), dim3(256), 0, st, g, ws.mean_part, ws.part, n_tiles);
        MCR_LAUNCH_CHECK("ds_backward_mean_kernel");
    }
    return 0;
}
