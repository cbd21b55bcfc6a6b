// The expansion layers of the depth decoder, for gfx950 -- the backward of expansion_layer.hip, in that file's notation.  near() is the
// nearest-source index, refl() the reflection index of pad 1, Ctot = Cmid + Cadd, c = cat(nearest(u), x_add).  Given d_y [B,Cout,H,W]:
//
//   g2 = d_y (y > 0 ? 1 : y + 1)                                   ELU'(z2) from y alone: below zero y = expm1(z2)
//   d_i_bias[co] = sum g2[b,co,i,j]
//   d_i_weight[co,k,di,dj] = sum_{b,i,j} g2[b,co,i,j] c[b,k,refl(i+di-1),refl(j+dj-1)]
//   G[b,k,P,Q] = sum_{co,di,dj} g2[b,co,P-di+1,Q-dj+1] i_weight[co,k,di,dj]          P in -1 .. H, Q in -1 .. W, g2 zero outside the image
//   d_c[b,k,i,j] = the sum of G over the padded cells (P,Q) with refl(P) = i, refl(Q) = j (up to four)
//   d_x_add = d_c[:, Cmid:],   d_u[b,m,s,t] = sum_{near(i) = s, near(j) = t} d_c[b,m,i,j],   g1 = d_u (u > 0 ? 1 : u + 1)
//   d_up_bias[m] = sum g1[b,m,s,t]
//   d_up_weight[ci,m,ki,kj] = sum_{b,s,t} x[b,ci,s,t] g1[b,m,s+ki-1,t+kj-1]          g1 zero outside h x w
//   d_x[b,ci,s,t] = sum_{m,ki,kj} g1[b,m,s+ki-1,t+kj-1] up_weight[ci,m,ki,kj]
//
// el_g2_kernel writes g2 to the arena once.  The two data gradients are launches of the forward's el_conv_kernel: G, a zero-padded
// correlation of g2 over an (H+2) x (W+2) domain, the source one row and one column earlier, i_weight read in the order of the transposed
// convolution's launch ([input channel][output channel], the taps flipped); d_x, a zero-padded correlation of g1 with up_weight in the
// convolution's order, unflipped.  Between them el_fold_kernel, a gather: a thread per element of d_x_add and of g1 adds the cells of G
// that reflect onto a pixel, over the contiguous range of pixels whose nearest source an element of u is (empty where the map shrinks: a
// zero, written), and multiplies by ELU'(u).  No scatter, no atomics.
//
// The two weight gradients are GEMMs over the pixels, K = B H W, on v_mfma_f32_16x16x4_f32: el_wgrad_kernel computes
//   D[ca,cb,t] = sum_{b,i,j} a[b,ca,i,j] s[b,cb,(i+di-1,j+dj-1)]
// with a the operand read at the pixel itself (g2; x) and s the one read through the forward's own offset table with its ring (c through
// refl and near; g1 zero-padded).  Per tap, D[16 ca x 16 cb] += A[16 ca x 4 pixels] B[4 pixels x 16 cb]: nine accumulators per 16 x 16
// block, a tenth for the bias gradient (the same instruction against a register of ones: on the a side for d_i_bias, on the s side at
// the centre tap for d_up_bias).  A workgroup of four waves stages 4 rows x 32 columns of one image at a time -- a [channels][128] and
// s [channels][6 x 34] -- through registers, the next tile on its way while this one is multiplied.  Two tiles: CHAN, 32 x 32 channels,
// a 16 x 16 block a wave, every wave all pixels; PIX, 16 x 16 channels, the four waves a row of the tile each, added through LDS in
// the order of the waves.  The pixel tiles are divided among `parts` workgroups per channel block (a function of the shape alone);
// each stores one partial per output into the arena, part-major, and el_wgrad_finish_kernel adds an output's partials in ascending
// order of the parts, in double.  No floating-point atomics: two calls give the same bits.
#include "expansion_layer.h"

namespace mcr {

__device__ __forceinline__ float el_elu_slope(float y) { return y > 0.f ? 1.f : y + 1.f; }      // ELU'(z) from y = ELU(z)

// grid (ceil(n / 256)): g2 = d_y ELU'(z2)
__global__ __launch_bounds__(256) void el_g2_kernel(const float* __restrict__ y, const float* __restrict__ d_y, float* __restrict__ g2, int n) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e < (unsigned)n) g2[e] = d_y[e] * el_elu_slope(y[e]);
}

// d_c of pixel (i, j) of one plane of G [(H+2) x (W+2)]: the cell itself, and along an axis padded -1 when i = 1, padded n when i = n - 2.
__device__ __forceinline__ float el_fold(const float* __restrict__ Gp, int i, int j, int H, int W) {
    const int W2 = W + 2;
    const int pr[3] = {i + 1, i == 1 ? 0 : -1, i == H - 2 ? H + 1 : -1}, qc[3] = {j + 1, j == 1 ? 0 : -1, j == W - 2 ? W + 1 : -1};
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (pr[a] >= 0 && qc[b] >= 0) s += Gp[pr[a] * W2 + qc[b]];
    return s;
}

// [lo, hi): the destinations d of 0 .. n_out-1 with el_nearest(d) = s (near is monotone), from an estimate corrected by the rule itself
__device__ __forceinline__ int el_first_dst(int s, float scale, int n_in, int n_out) {
    int d = (int)fminf((float)s / scale, (float)n_out);
    while (d > 0 && el_nearest(d - 1, scale, n_in) >= s) --d;
    while (d < n_out && el_nearest(d, scale, n_in) < s) ++d;
    return d;
}

// grid (blocks_u + blocks_a), 256 threads, a thread per element: the first blocks_u blocks g1 [B,Cmid,h,w] (g1 NULL: blocks_u = 0), the
// others d_x_add [B,Cadd,H,W].  G [B,Ctot,H+2,W+2].
__global__ __launch_bounds__(256) void el_fold_kernel(const float* __restrict__ G, const float* __restrict__ u, float* __restrict__ g1,
                                                      float* __restrict__ d_x_add, int n_u, int n_a, int Cmid, int Cadd, int h, int w, int H,
                                                      int W, float sy, float sx, int blocks_u) {
    const int Ctot = Cmid + Cadd;
    const size_t gplane = (size_t)(H + 2) * (W + 2);
    if ((int)blockIdx.x < blocks_u) {
        const unsigned eu = blockIdx.x * 256u + threadIdx.x;
        if (eu >= (unsigned)n_u) return;
        const int e = (int)eu;
        const int t = e % w, s = (e / w) % h, bm = e / (w * h), m = bm % Cmid, b = bm / Cmid;
        const int i0 = el_first_dst(s, sy, h, H), i1 = el_first_dst(s + 1, sy, h, H);
        const int j0 = el_first_dst(t, sx, w, W), j1 = el_first_dst(t + 1, sx, w, W);
        const float* Gp = G + ((size_t)b * Ctot + m) * gplane;
        float d_u = 0.f;
        for (int i = i0; i < i1; ++i)
            for (int j = j0; j < j1; ++j) d_u += el_fold(Gp, i, j, H, W);
        g1[e] = d_u * el_elu_slope(u[e]);
    } else {
        const unsigned ea = (blockIdx.x - blocks_u) * 256u + threadIdx.x;
        if (ea >= (unsigned)n_a) return;
        const int e = (int)ea;
        const int j = e % W, i = (e / W) % H, ba = e / (W * H), a = ba % Cadd, b = ba / Cadd;
        d_x_add[e] = el_fold(G + ((size_t)b * Ctot + Cmid + a) * gplane, i, j, H, W);
    }
}

constexpr int EW_TH = 4, EW_TW = 32;                 // the pixel tile of the weight-gradient kernel

// grid (parts, ca_blocks cb_blocks), 256 threads.  a [B,CA,H,W]; src0 [B,C0,h0,w0] and src1 [B,C1,H,W] the CB = C0 + C1 channels of s, as
// in el_conv_kernel (ZPAD: src0 zero-padded, h0 x w0 = H x W; otherwise the convolution's table).  part[n][o], n = blockIdx.x:
// o = (ca CB + cb) 9 + t, and from o = 9 CA CB on the bias gradient: BIAS 1 of the a side (CA values, stored by cb block 0), BIAS 2 of the s
// side (CB values, stored by ca block 0).  A workgroup's tile is 16 WA x 16 WB channels; WP waves divide the rows of a pixel tile.
// Workgroup n owns the pixel tiles n per .. min(units, (n + 1) per) - 1 of the B tiles units.
template <bool ZPAD, int BIAS, int WA, int WB, int WP>
__global__ __launch_bounds__(256) void el_wgrad_kernel(const float* __restrict__ a, const float* __restrict__ src0, const float* __restrict__ src1,
                                                       float* __restrict__ part, int CA, int C0, int C1, int h0, int w0, int H, int W, float sy,
                                                       float sx, int tiles_x, int tiles, int units, int per, int cb_blocks, int n_out) {
    constexpr int NT = 256, TH = EW_TH, TW = EW_TW, NP = TH * TW, RW = TW + 2, R = RW * (TH + 2), AS = el_pad4(NP), RS = el_pad4(R);
    constexpr int CA_T = 16 * WA, CB_T = 16 * WB, KA = CA_T * NP / NT, KS = (CB_T * R + NT - 1) / NT;
    constexpr int XS = CA_T * AS, STAGE = XS + CB_T * RS, BLK = 16 * 16 * 9, RED = 4 * BLK + 4 * 16, SM = STAGE > RED ? STAGE : RED;
    static_assert(WA * WB * WP == 4 && TH % WP == 0 && (CA_T * NP) % NT == 0, "four waves; the rows divide among them");
    __shared__ float sm[SM];
    __shared__ int off0[R], off1[R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lk = lane >> 4, lp = lane & 15;
    const int wa = wave % WA, wb = (wave / WA) % WB, wp = wave / (WA * WB);
    const int ca0 = (blockIdx.y / cb_blocks) * CA_T, cb0 = (blockIdx.y % cb_blocks) * CB_T;
    const int CB = C0 + C1;
    const size_t plane0 = (size_t)h0 * w0, plane1 = (size_t)H * W;
    const int u0 = blockIdx.x * per, u1 = min(units, u0 + per);

    // A tile travels through registers, every load in flight at once and from an address that exists: va element e = ca NP + ty TW + tx, vs
    // element e = cb R + r through the table.
    float va[KA], vs[KS];
    auto load = [&](int unit) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));                              // the staging indices are recomputed per tile, not kept in registers across the loop
        const int b = unit / tiles, tile = unit - b * tiles;
        const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int e = tid + k * NT;
            const int ca = e / NP, p = e - ca * NP, i = y0 + p / TW, j = x0 + p % TW;
            const bool live = ca0 + ca < CA && i < H && j < W;
            const float v = a[live ? ((size_t)b * CA + ca0 + ca) * plane1 + (size_t)i * W + j : 0];
            va[k] = live ? v : 0.f;
        }
        const float* s0 = src0 + (size_t)b * C0 * plane0;
        const float* s1 = C1 ? src1 + (size_t)b * C1 * plane1 : src0;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int e = tid + k * NT;
            const int c = e / R, r = e - c * R, cc = cb0 + c;
            const bool in0 = cc < C0, live = e < CB_T * R && cc < CB;
            const int o = live ? (in0 ? off0[r] : off1[r]) : -1;
            const float* p = !live ? s0 : in0 ? s0 + (size_t)cc * plane0 : s1 + (size_t)(cc - C0) * plane1;
            const float v = p[o < 0 ? 0 : o];
            vs[k] = o < 0 ? 0.f : v;
        }
    };
    auto table = [&](int unit) {
        const int tile = unit % tiles;
        el_fill_table<ZPAD, 0>(off0, off1, R, RW, (tile / tiles_x) * TH, (tile % tiles_x) * TW, h0, w0, H, W, sy, sx, tid, NT);
    };

    el_f32x4 acc[10];
#pragma unroll
    for (int n = 0; n < 10; ++n) acc[n] = el_f32x4{0.f, 0.f, 0.f, 0.f};
    // a wave whose block of channels lies past the end has nothing to multiply (wave-uniform)
    const bool active = ca0 + wa * 16 < CA && cb0 + wb * 16 < CB;
    const bool with_bias = BIAS == 1 ? cb0 == 0 && wb == 0 : BIAS == 2 ? ca0 == 0 && wa == 0 : false;

    if (u0 < u1) {
        table(u0);
        __syncthreads();
        load(u0);
    }
    for (int unit = u0; unit < u1; ++unit) {
        __syncthreads();                                           // the tile before this one has been multiplied
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            const int e = tid + k * NT;
            sm[(e / NP) * AS + e % NP] = va[k];
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int e = tid + k * NT;
            if (e < CB_T * R) sm[XS + (e / R) * RS + e % R] = vs[k];
        }
        if (unit + 1 < u1) table(unit + 1);                        // every load through the table of this tile has returned: its values are stored
        __syncthreads();
        if (unit + 1 < u1) load(unit + 1);                         // the next tile is on its way while this one is multiplied
        if (!active) continue;
        for (int ty = wp; ty < TH; ty += WP) {
            const float* ap = sm + (wa * 16 + lp) * AS + ty * TW + lk;
            const float* sp = sm + XS + (wb * 16 + lp) * RS + ty * RW + lk;
#pragma unroll 2
            for (int xg = 0; xg < TW / 4; ++xg) {
                const float av = ap[xg * 4];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const float sv = sp[(t / 3) * RW + xg * 4 + t % 3];
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sv, acc[t], 0, 0, 0);
                }
                if (BIAS == 1 && with_bias) acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, acc[9], 0, 0, 0);
                if (BIAS == 2 && with_bias) acc[9] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, sp[RW + xg * 4 + 1], acc[9], 0, 0, 0);
            }
        }
    }

    // The accumulators go through LDS: element j of lane l of accumulator t is (ca = (l >> 4) 4 + j, cb = l & 15); a wave's block lies as
    // [ca][cb][t], so that the 9 x 16 values of a ca are consecutive in memory as well.  The bias sums: a side, column 0 of accumulator 9
    // (ca = (l >> 4) 4 + j); s side, its row 0 (cb = l).
    __syncthreads();
    float* bs = sm + 4 * BLK;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[wave * BLK + ((lk * 4 + j) * 16 + lp) * 9 + t] = acc[t][j];
    if (BIAS == 1 && lp == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bs[wave * 16 + lk * 4 + j] = acc[9][j];
    }
    if (BIAS == 2 && lk == 0) bs[wave * 16 + lp] = acc[9][0];
    __syncthreads();
    float* dst = part + (size_t)blockIdx.x * n_out;
    for (int e = tid; e < WA * WB * BLK; e += NT) {
        const int q = e / BLK, r = e - q * BLK, ca = r / 144, rem = r - ca * 144, cb = rem / 9;
        float v = sm[q * BLK + r];                                 // wave q of the first row group: (wa, wb) = (q % WA, q / WA)
#pragma unroll
        for (int p = 1; p < WP; ++p) v += sm[(q + p * WA * WB) * BLK + r];
        const int gca = ca0 + (q % WA) * 16 + ca, gcb = cb0 + (q / WA) * 16 + cb;
        if (gca < CA && gcb < CB) dst[((size_t)gca * CB + gcb) * 9 + (rem - cb * 9)] = v;
    }
    if (BIAS == 1 && cb0 == 0 && tid < CA_T) {                     // the waves with wb = 0: wave = wa + WA WB p
        float v = bs[(tid / 16) * 16 + tid % 16];
#pragma unroll
        for (int p = 1; p < WP; ++p) v += bs[(tid / 16 + p * WA * WB) * 16 + tid % 16];
        if (ca0 + tid < CA) dst[(size_t)CA * CB * 9 + ca0 + tid] = v;
    }
    if (BIAS == 2 && ca0 == 0 && tid < CB_T) {                     // the waves with wa = 0: wave = WA wb + WA WB p
        float v = bs[(tid / 16) * WA * 16 + tid % 16];
#pragma unroll
        for (int p = 1; p < WP; ++p) v += bs[((tid / 16) * WA + p * WA * WB) * 16 + tid % 16];
        if (cb0 + tid < CB) dst[(size_t)CA * CB * 9 + cb0 + tid] = v;
    }
}

// grid (ceil(n_out / 64)), 256 threads: output o = 64 blockIdx.x + (tid & 63); quarter q = tid >> 6 of the workgroup adds the parts q,
// q + 4, .. ascending, in double, and the four quarters are added in the one fixed association.  The first n_w outputs go to d_weight,
// the others to d_bias; a NULL destination is not written.
__global__ __launch_bounds__(256) void el_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ d_weight,
                                                              float* __restrict__ d_bias, int n_w, int n_out, int parts) {
    __shared__ double red[4][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6, o = blockIdx.x * 64 + l;
    double acc = 0.0;
    if (o < n_out)
        for (int n = q; n < parts; n += 4) acc += (double)part[(size_t)n * n_out + o];
    red[q][l] = acc;
    __syncthreads();
    if (q != 0 || o >= n_out) return;
    const float v = (float)four_wave_sum(&red[0][l], 64);
    if (o < n_w) {
        if (d_weight) d_weight[o] = v;
    } else if (d_bias) {
        d_bias[o - n_w] = v;
    }
}

// The tile of a weight-gradient pass and its division of the pixels, functions of the shape alone.  PIX where a side has no more than 16
// channels (upstream's expansion1: the 32-channel tile would multiply zeros in three waves of four), CHAN otherwise.  parts: as many
// workgroups per channel block as bring the launch to about four per compute unit, at most one per pixel tile.
struct ElWgradPlan { bool pix; int tiles_x, tiles, units, per, parts, ca_blocks, cb_blocks; size_t n_out; };
static ElWgradPlan el_wgrad_plan(int64_t B, int64_t CA, int64_t CB, int64_t n_bias, int64_t H, int64_t W) {
    ElWgradPlan p;
    p.pix = CA <= 16 || CB <= 16;
    const int ct = p.pix ? 16 : 32;
    p.ca_blocks = (int)cdiv(CA, ct), p.cb_blocks = (int)cdiv(CB, ct);
    p.tiles_x = (int)cdiv(W, EW_TW), p.tiles = p.tiles_x * (int)cdiv(H, EW_TH);
    const int64_t units = B * p.tiles, want = cdiv(1024, (int64_t)p.ca_blocks * p.cb_blocks);
    const int64_t per = cdiv(units, units < want ? units : want);
    p.units = (int)units, p.per = (int)per, p.parts = (int)cdiv(units, per);
    p.n_out = (size_t)(CA * CB * 9 + n_bias);
    return p;
}

// BIAS 1: a = g2 against c (the convolution's table), d_i_weight and d_i_bias; BIAS 2: a = x against g1 (zero-padded), d_up_weight and d_up_bias
template <bool ZPAD, int BIAS>
static void el_wgrad_launch(hipStream_t st, const ElWgradPlan& p, const float* a, const float* src0, const float* src1, float* part, int CA,
                            int C0, int C1, int h0, int w0, int H, int W) {
    const dim3 grid((unsigned)p.parts, (unsigned)(p.ca_blocks * p.cb_blocks));
    const float sy = (float)h0 / (float)H, sx = (float)w0 / (float)W;
    if (p.pix)
        hipLaunchKernelGGL((el_wgrad_kernel<ZPAD, BIAS, 1, 1, 4>), grid, dim3(256), 0, st, a, src0, src1, part, CA, C0, C1, h0, w0, H, W, sy, sx,
                           p.tiles_x, p.tiles, p.units, p.per, p.cb_blocks, (int)p.n_out);
    else
        hipLaunchKernelGGL((el_wgrad_kernel<ZPAD, BIAS, 2, 2, 1>), grid, dim3(256), 0, st, a, src0, src1, part, CA, C0, C1, h0, w0, H, W, sy, sx,
                           p.tiles_x, p.tiles, p.units, p.per, p.cb_blocks, (int)p.n_out);
}

static bool el_bwd_sizes_ok(int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h, int64_t w, int64_t H, int64_t W) {
    return el_sizes_ok(B, Cin, Cmid, Cadd, Cout, h, w, H, W) && H + 2 <= 0x7fffffffll && W + 2 <= 0x7fffffffll &&
           el_fits(B, Cmid + Cadd, H + 2, W + 2);               // G, the largest tensor of the arena
}

// g2 [B,Cout,H,W]; G [B,Ctot,H+2,W+2]; g1 [B,Cmid,h,w]; part: the partials of one weight-gradient pass at a time, [parts][outputs]
struct ElBwdScratch { float *g2, *G, *g1, *part; };
static ElBwdScratch carve_expansion_bwd(Arena& a, int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h, int64_t w,
                                        int64_t H, int64_t W) {
    ElBwdScratch s;
    const int64_t Ctot = Cmid + Cadd;
    s.g2 = a.f((size_t)(B * Cout * H * W));
    s.G = a.f((size_t)(B * Ctot * (H + 2) * (W + 2)));
    s.g1 = a.f((size_t)(B * Cmid * h * w));
    const ElWgradPlan pi = el_wgrad_plan(B, Cout, Ctot, Cout, H, W), pu = el_wgrad_plan(B, Cin, Cmid, Cmid, h, w);
    const size_t ni = pi.n_out * pi.parts, nu = pu.n_out * pu.parts;
    s.part = a.f(ni > nu ? ni : nu);
    return s;
}

}  // namespace mcr

using namespace mcr;

extern "C" size_t mcr_expansion_layer_backward_workspace_bytes(int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h,
                                                               int64_t w, int64_t H, int64_t W) {
    if (!el_bwd_sizes_ok(B, Cin, Cmid, Cadd, Cout, h, w, H, W)) return 0;
    return measure(carve_expansion_bwd, B, Cin, Cmid, Cadd, Cout, h, w, H, W);
}

extern "C" int mcr_expansion_layer_backward(const float* x, const float* x_add, const float* up_weight, const float* i_weight, const float* u,
                                            const float* y, const float* d_y, float* d_x, float* d_x_add, float* d_up_weight,
                                            float* d_up_bias, float* d_i_weight, float* d_i_bias, int64_t B, int Cin, int Cmid, int Cadd,
                                            int Cout, int h, int w, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_expansion_layer_backward";
    if (int e = el_check_sizes(who, B, Cin, Cmid, Cadd, Cout, h, w, H, W)) return e;
    MCR_REQUIRE(el_bwd_sizes_ok(B, Cin, Cmid, Cadd, Cout, h, w, H, W),
                "%s: B = %lld, %d + %d channels, %d x %d with its ring: a tensor has 2^31 elements or more", who, (long long)B, Cmid, Cadd, H, W);
    MCR_REQUIRE(d_x || d_x_add || d_up_weight || d_up_bias || d_i_weight || d_i_bias, "%s: all six outputs are NULL, nothing to do", who);
    MCR_REQUIRE(x && up_weight && i_weight && u && y && d_y && (Cadd == 0 || x_add), "%s: NULL operand", who);
    MCR_REQUIRE(Cadd > 0 || !d_x_add, "%s: d_x_add with Cadd = 0, there is no x_add", who);
    if (int e = check_workspace(who, workspace, workspace_bytes,
                                mcr_expansion_layer_backward_workspace_bytes(B, Cin, Cmid, Cadd, Cout, h, w, H, W)))
        return e;
    Arena arena{(char*)workspace, workspace_bytes};
    const ElBwdScratch ws = carve_expansion_bwd(arena, B, Cin, Cmid, Cadd, Cout, h, w, H, W);
    const hipStream_t st = (hipStream_t)stream;
    const int Ctot = Cmid + Cadd;
    const bool want_i = d_i_weight || d_i_bias, want_up = d_up_weight || d_up_bias, want_g1 = d_x || want_up, want_G = want_g1 || d_x_add;

    const int n_y = (int)(B * Cout * H * W);
    hipLaunchKernelGGL(el_g2_kernel, dim3((unsigned)cdiv(n_y, 256)), dim3(256), 0, st, y, d_y, ws.g2, n_y);
    MCR_LAUNCH_CHECK("el_g2_kernel");
    if (want_i) {
        const ElWgradPlan p = el_wgrad_plan(B, Cout, Ctot, Cout, H, W);
        el_wgrad_launch<false, 1>(st, p, ws.g2, u, Cadd ? x_add : nullptr, ws.part, Cout, Cmid, Cadd, h, w, H, W);
        MCR_LAUNCH_CHECK("el_wgrad_kernel (convolution)");
        hipLaunchKernelGGL(el_wgrad_finish_kernel, dim3((unsigned)cdiv(p.n_out, 64)), dim3(256), 0, st, ws.part, d_i_weight, d_i_bias,
                           Cout * Ctot * 9, (int)p.n_out, p.parts);
        MCR_LAUNCH_CHECK("el_wgrad_finish_kernel (convolution)");
    }
    if (want_G) {
        el_launch<true, 1>(st, ws.g2, nullptr, i_weight, nullptr, ws.G, B, Cout, 0, H, W, Ctot, H + 2, W + 2);
        MCR_LAUNCH_CHECK("el_conv_kernel (G)");
        const int n_u = want_g1 ? (int)(B * Cmid * h * w) : 0, n_a = d_x_add ? (int)(B * Cadd * H * W) : 0;
        const int blocks_u = (int)cdiv(n_u, 256);
        hipLaunchKernelGGL(el_fold_kernel, dim3((unsigned)(blocks_u + cdiv(n_a, 256))), dim3(256), 0, st, ws.G, u, ws.g1, d_x_add, n_u, n_a, Cmid,
                           Cadd, h, w, H, W, (float)h / (float)H, (float)w / (float)W, blocks_u);
        MCR_LAUNCH_CHECK("el_fold_kernel");
    }
    if (want_up) {
        const ElWgradPlan p = el_wgrad_plan(B, Cin, Cmid, Cmid, h, w);
        el_wgrad_launch<true, 2>(st, p, x, ws.g1, nullptr, ws.part, Cin, Cmid, 0, h, w, h, w);
        MCR_LAUNCH_CHECK("el_wgrad_kernel (transposed convolution)");
        hipLaunchKernelGGL(el_wgrad_finish_kernel, dim3((unsigned)cdiv(p.n_out, 64)), dim3(256), 0, st, ws.part, d_up_weight, d_up_bias,
                           Cin * Cmid * 9, (int)p.n_out, p.parts);
        MCR_LAUNCH_CHECK("el_wgrad_finish_kernel (transposed convolution)");
    }
    if (d_x) {
        el_launch<false, 2>(st, ws.g1, nullptr, up_weight, nullptr, d_x, B, Cmid, 0, h, w, Cin, h, w);
        MCR_LAUNCH_CHECK("el_conv_kernel (d_x)");
    }
    return 0;
}
