// What the forward (expansion_layer.hip) and the backward (expansion_layer_bwd.hip) of the decoder's expansion layers share: the 3 x 3
// correlation kernel on v_mfma_f32_16x16x4_f32 with its table of source offsets, the reflection and nearest-source indices, the tile
// choice and the size checks.  The notation is that of expansion_layer.hip's header.
#pragma once
#include "workspace.h"
#include <math.h>

namespace mcr {

constexpr int EL_MAX_C = 512;

typedef float el_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float el_elu(float z) { return z > 0.f ? z : expm1f(z); }
__device__ __forceinline__ int el_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // i in -1 .. n, n >= 2
__device__ __forceinline__ int el_nearest(int dst, float scale, int n_in) { return min((int)floorf((float)dst * scale), n_in - 1); }

constexpr int el_pad16(int n) { return n + ((16 - n % 32) + 32) % 32; }                 // the next n' >= n with n' = 16 mod 32
constexpr int el_pad2(int n) { return n + ((2 - n % 32) + 32) % 32; }                   // ... with n' = 2 mod 32
constexpr int el_pad4(int n) { return n + ((4 - n % 32) + 32) % 32; }                   // ... with n' = 4 mod 32

// The table of a staged region of RW columns whose cell (0,0) is the padded coordinate (y0 - 1, x0 - 1) of an H x W domain: cell
// r = ry RW + rx is the padded coordinate (y0 - 1 + ry, x0 - 1 + rx); off0[r] / off1[r] say where it comes from in a plane of src0
// [h0 x w0] and of src1 [H x W], -1 for a zero.  ZPAD: a zero-padded source, src0 alone, read SHIFT rows and columns earlier (the
// transposed convolution's launch, SHIFT 0 and h0 x w0 = H x W; the backward's correlations); otherwise the convolution's: the reflection
// index, src0 through the nearest-source index besides (a coordinate past the mirror, which no pixel of the image reads, is a zero).
template <bool ZPAD, int SHIFT>
__device__ __forceinline__ void el_fill_table(int* off0, int* off1, int R, int RW, int y0, int x0, int h0, int w0, int H, int W, float sy,
                                              float sx, int tid, int NT) {
    for (int r = tid; r < R; r += NT) {
        const int ry = r / RW, rx = r - ry * RW;
        const int cy = y0 - 1 + ry, cx = x0 - 1 + rx;              // >= -1
        int o0 = -1, o1 = -1;
        if (ZPAD) {
            const int qy = cy - SHIFT, qx = cx - SHIFT;
            if (qy >= 0 && qy < h0 && qx >= 0 && qx < w0) o0 = qy * w0 + qx;
        } else if (cy <= H && cx <= W) {
            const int my = el_reflect(cy, H), mx = el_reflect(cx, W);
            o1 = my * W + mx;
            o0 = el_nearest(my, sy, h0) * w0 + el_nearest(mx, sx, w0);
        }
        off0[r] = o0, off1[r] = o1;
    }
}

// grid (B co_blocks tiles), 256 threads.  src0 [B,C0,h0,w0] and src1 [B,C1,H,W] (C1 = 0: absent) are the virtual input's channels
// 0 .. C0-1 and C0 .. C0+C1-1; out [B,Cout,H,W].  UP: the weight is [C0,Cout,3,3] and its taps are flipped; otherwise it is
// [Cout,C0+C1,3,3].  BWD 0, the forward: UP is the transposed convolution's launch (h0 x w0 = H x W, zero padding), the other the
// convolution's (reflection, src0 through the nearest index with scales sy = h0 / H, sx = w0 / W); bias and ELU in the epilogue.  BWD 1 and
// 2, the backward's two data gradients: zero padding with either weight order, no bias, no ELU; BWD 1 reads the source one row and one
// column earlier (an (h0 + 2) x (w0 + 2) output over an h0 x w0 source).  AFFINE, the ResNet basic block's convolutions (basic_block.hip):
// zero padding with the convolution's weight order, and the epilogue `epi` instead of bias and ELU -- an eval-mode BatchNorm as a scale
// and a shift per output channel, an optional residual, ReLU.  The other instantiations do not read `epi`.
struct ElAffine {
    const float *bn_weight, *bn_bias, *bn_mean, *bn_var;   // torch's four vectors [Cout]
    const float* residual;                                 // [B,Cout,H,W] added after the BatchNorm, or NULL
    float eps;
};
// a = weight / sqrt(var + eps) and b = bias - mean a of channel c, in float: the same expressions as resnet_stem.hip's
__device__ __forceinline__ void el_affine_of(const ElAffine& e, int c, float& a, float& b) {
    a = e.bn_weight[c] * (1.0f / sqrtf(e.bn_var[c] + e.eps));
    b = fmaf(-e.bn_mean[c], a, e.bn_bias[c]);
}

template <bool UP, int TH, int NSEG, int MA, int WK, int KC, int BWD = 0, bool AFFINE = false>
__global__ __launch_bounds__(256) void el_conv_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                      const float* __restrict__ weight, const float* __restrict__ bias, float* __restrict__ out,
                                                      int C0, int C1, int h0, int w0, int Cout, int H, int W, float sy, float sx, int tiles_x,
                                                      int tiles, int co_blocks, ElAffine epi) {
    constexpr int NT = 256, WP = 4 / WK, ROWS = TH / WP, TW = 16 * NSEG, RW = TW + 2, R = RW * (TH + 2), RS = el_pad16(R);
    constexpr int CO_T = 16 * MA, CS = el_pad2(KC * 9), NACC = ROWS * NSEG * MA;
    constexpr int XS = KC * RS, WN = CO_T * KC * 9, KI = (KC * R + NT - 1) / NT, KW = (WN + NT - 1) / NT;
    constexpr int RED = 4 * NACC * 256, SM = XS + CO_T * CS > RED ? XS + CO_T * CS : RED;
    static_assert(TH % WP == 0 && KC % (4 * WK) == 0 && NACC >= 2, "rows divide among the waves, channel groups among the waves, two chains");
    __shared__ float sm[SM];
    __shared__ int off0[R], off1[R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kw = wave % WK, wp = wave / WK, lk = lane >> 4, lp = lane & 15;
    int bid = blockIdx.x;
    const int tile = bid % tiles;
    bid /= tiles;
    const int co0 = (bid % co_blocks) * CO_T, b = bid / co_blocks;
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int Ctot = C0 + C1;
    const size_t plane0 = (size_t)h0 * w0, plane1 = (size_t)H * W;
    const float* s0 = src0 + (size_t)b * C0 * plane0;
    const float* s1 = C1 ? src1 + (size_t)b * C1 * plane1 : src0;

    el_fill_table<UP || BWD != 0 || AFFINE, BWD == 1 ? 1 : 0>(off0, off1, R, RW, y0, x0, h0, w0, H, W, sy, sx, tid, NT);
    __syncthreads();

    // A chunk of KC channels travels through registers, every load in flight at once and from an address that exists (what is absent is
    // read at offset 0 and replaced by zero): vi the region, element e = c R + r; vw the weights in the order they lie in memory,
    // element e = co (KC 9) + c 9 + t of weight[co0 + co][c0 + c][t], or for UP e = c (CO_T 9) + co 9 + t' of weight[c0 + c][co0 + co][t'],
    // whose tap is t = 8 - t' (both axes flipped).
    float vi[KI], vw[KW];
    auto load = [&](int c0) {
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int e = tid + k * NT;
            const int c = e / R, r = e - c * R, cc = c0 + c;
            const bool in0 = cc < C0, live = e < KC * R && cc < Ctot;
            const int o = live ? (in0 ? off0[r] : off1[r]) : -1;
            const float* p = !live ? s0 : in0 ? s0 + (size_t)cc * plane0 : s1 + (size_t)(cc - C0) * plane1;
            const float v = p[o < 0 ? 0 : o];
            vi[k] = o < 0 ? 0.f : v;
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int e = tid + k * NT;
            int co, c, rr;
            if (UP) {
                c = e / (CO_T * 9), rr = e - c * (CO_T * 9), co = rr / 9;
            } else {
                co = e / (KC * 9), rr = e - co * (KC * 9), c = rr / 9;
            }
            const bool live = e < WN && co0 + co < Cout && c0 + c < Ctot;
            const size_t at = UP ? ((size_t)(c0 + c) * Cout + co0) * 9 + rr : ((size_t)(co0 + co) * Ctot + c0) * 9 + rr;
            const float v = weight[live ? at : 0];
            vw[k] = live ? v : 0.f;
        }
    };

    el_f32x4 acc[NACC];
#pragma unroll
    for (int n = 0; n < NACC; ++n) acc[n] = el_f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int c0 = 0; c0 < Ctot; c0 += KC) {
        __syncthreads();                                           // the chunk before this one has been multiplied
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int e = tid + k * NT;
            const int c = e / R, r = e - c * R;
            if (e < KC * R) sm[c * RS + r] = vi[k];
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int e = tid + k * NT;
            int co, c, t;
            if (UP) {
                c = e / (CO_T * 9);
                const int rr = e - c * (CO_T * 9);
                co = rr / 9, t = 8 - (rr - co * 9);
            } else {
                co = e / (KC * 9);
                const int rr = e - co * (KC * 9);
                c = rr / 9, t = rr - c * 9;
            }
            if (e < WN) sm[XS + co * CS + c * 9 + t] = vw[k];
        }
        __syncthreads();
        if (c0 + KC < Ctot) load(c0 + KC);                         // the next chunk is on its way while this one is multiplied
        const int groups = (min(KC, Ctot - c0) + 3) >> 2;          // of four channels; the tail of the last one is zeros
        for (int g = kw; g < groups; g += WK) {
            const float* xb = sm + (g * 4 + lk) * RS + (wp * ROWS) * RW + lp;
            const float* ab = sm + XS + lp * CS + (g * 4 + lk) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int di = t / 3, dj = t % 3;
                float a[MA];
#pragma unroll
                for (int m = 0; m < MA; ++m) a[m] = ab[m * 16 * CS + t];
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int s = 0; s < NSEG; ++s) {
                        const float bv = xb[(r + di) * RW + s * 16 + dj];
#pragma unroll
                        for (int m = 0; m < MA; ++m)
                            acc[(r * NSEG + s) * MA + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bv, acc[(r * NSEG + s) * MA + m], 0, 0, 0);
                    }
            }
        }
    }

    // The accumulators go through LDS: element j of lane l of accumulator n is output channel m 16 + (l >> 4) 4 + j at pixel
    // (row wp ROWS + r, column s 16 + (l & 15)).  A thread then owns pixels along a row, adds the WK partial sums in the order of the
    // waves, the bias last, and stores.
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NACC; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[((wave * NACC + n) * 4 + j) * 64 + lane] = acc[n][j];
    if (AFFINE) {                                                  // scale and shift once per channel, in the tables nobody reads any more
        static_assert(!AFFINE || CO_T <= R, "a table entry per output channel of the tile");
        if (tid < CO_T && co0 + tid < Cout) {
            float a, sh;
            el_affine_of(epi, co0 + tid, a, sh);
            off0[tid] = __float_as_int(a), off1[tid] = __float_as_int(sh);
        }
    }
    __syncthreads();
    float* ob = out + (size_t)b * Cout * plane1;
    for (int o = tid; o < CO_T * TH * TW; o += NT) {
        const int co = o / (TH * TW), p = o - co * (TH * TW);
        const int ty = p / TW, tx = p - ty * TW;
        const int n = ((ty % ROWS) * NSEG + tx / 16) * MA + co / 16, l = ((co % 16) / 4) * 16 + tx % 16, j = co % 4;
        const int w0_ = (ty / ROWS) * WK;
        float z = sm[((w0_ * NACC + n) * 4 + j) * 64 + l];
#pragma unroll
        for (int q = 1; q < WK; ++q) z += sm[(((w0_ + q) * NACC + n) * 4 + j) * 64 + l];
        const int i = y0 + ty, jx = x0 + tx;
        if (co0 + co < Cout && i < H && jx < W) {
            const size_t at = (size_t)(co0 + co) * plane1 + (size_t)i * W + jx;
            if (AFFINE) {
                float v = fmaf(z, __int_as_float(off0[co]), __int_as_float(off1[co]));
                if (epi.residual) v += epi.residual[(size_t)b * Cout * plane1 + at];
                ob[at] = fmaxf(v, 0.f);
            } else {
                ob[at] = BWD ? z : el_elu(z + bias[co0 + co]);
            }
        }
    }
}

// The three tiles.  ROWS: 4 rows x 32 columns, a row a wave, for 16 output channels where there are no more (upstream's expansion1), for 32
// otherwise.  SPLIT: 2 rows x 16 columns x 16 output channels with the channels of a chunk of 32 divided among the waves, where the
// 32-channel tile would give the machine fewer workgroups than it has compute units.
enum ElTile { EL_ROWS16, EL_ROWS32, EL_SPLIT };
static ElTile el_tile(int64_t B, int Cout, int H, int W) {
    if (Cout <= 16) return EL_ROWS16;
    return B * cdiv(Cout, 32) * cdiv(H, 4) * cdiv(W, 32) < 256 ? EL_SPLIT : EL_ROWS32;
}

template <bool UP, int BWD, int TH, int NSEG, int MA, int WK, int KC, bool AFFINE = false>
static void el_launch_as(hipStream_t st, const float* src0, const float* src1, const float* weight, const float* bias, float* out, int64_t B,
                         int C0, int C1, int h0, int w0, int Cout, int H, int W, ElAffine epi = ElAffine{}) {
    const int tx = (int)cdiv(W, 16 * NSEG), tiles = tx * (int)cdiv(H, TH), cob = (int)cdiv(Cout, 16 * MA);
    hipLaunchKernelGGL((el_conv_kernel<UP, TH, NSEG, MA, WK, KC, BWD, AFFINE>), dim3((unsigned)(B * cob * tiles)), dim3(256), 0, st, src0, src1, weight,
                       bias, out, C0, C1, h0, w0, Cout, H, W, (float)h0 / (float)H, (float)w0 / (float)W, tx, tiles, cob, epi);
}

template <bool UP, int BWD = 0>
static void el_launch(hipStream_t st, const float* src0, const float* src1, const float* weight, const float* bias, float* out, int64_t B, int C0,
                      int C1, int h0, int w0, int Cout, int H, int W) {
    switch (el_tile(B, Cout, H, W)) {
        case EL_ROWS16: el_launch_as<UP, BWD, 4, 2, 1, 1, 16>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
        case EL_ROWS32: el_launch_as<UP, BWD, 4, 2, 2, 1, 16>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
        case EL_SPLIT: el_launch_as<UP, BWD, 2, 1, 1, 4, 32>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
    }
}

static bool el_fits(int64_t B, int64_t C, int64_t H, int64_t W) { return H * W <= 0x7fffffffll && B <= 0x7fffffffll / (C * H * W); }

static bool el_sizes_ok(int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h, int64_t w, int64_t H, int64_t W) {
    if (B < 1 || Cin < 1 || Cin > EL_MAX_C || Cmid < 1 || Cmid > EL_MAX_C || Cout < 1 || Cout > EL_MAX_C) return false;
    if (Cadd < 0 || Cmid + Cadd > EL_MAX_C || h < 1 || w < 1 || H < 2 || W < 2) return false;
    if (h > 0x7fffffffll || w > 0x7fffffffll || H > 0x7fffffffll || W > 0x7fffffffll) return false;
    return el_fits(B, Cin, h, w) && el_fits(B, Cmid, h, w) && el_fits(B, Cout, H, W) && (Cadd == 0 || el_fits(B, Cadd, H, W));
}

// The forward entry's refusals of sizes, shared with the backward's: `who` is the entry's name.
static int el_check_sizes(const char* who, int64_t B, int Cin, int Cmid, int Cadd, int Cout, int h, int w, int H, int W) {
    MCR_REQUIRE(H >= 2 && W >= 2, "%s: the output is %d x %d, H and W must be at least 2 (the reflection padding)", who, H, W);
    MCR_REQUIRE(h >= 1 && w >= 1, "%s: the input is %d x %d, h and w must be at least 1", who, h, w);
    MCR_REQUIRE(Cin >= 1 && Cin <= EL_MAX_C && Cmid >= 1 && Cmid <= EL_MAX_C && Cout >= 1 && Cout <= EL_MAX_C,
                "%s: Cin = %d, Cmid = %d, Cout = %d channels, 1 .. %d are supported", who, Cin, Cmid, Cout, EL_MAX_C);
    MCR_REQUIRE(Cadd >= 0 && Cmid + Cadd <= EL_MAX_C, "%s: Cmid + Cadd = %d + %d channels, Cadd >= 0 and at most %d together are supported", who,
                Cmid, Cadd, EL_MAX_C);
    MCR_REQUIRE(B >= 1, "%s: B = %lld must be at least 1", who, (long long)B);
    MCR_REQUIRE(el_sizes_ok(B, Cin, Cmid, Cadd, Cout, h, w, H, W),
                "%s: B = %lld, channels %d %d %d %d, %d x %d -> %d x %d: a tensor has 2^31 elements or more", who, (long long)B, Cin, Cmid, Cadd,
                Cout, h, w, H, W);
    return 0;
}

struct ElScratch { float* u; };                        // [B,Cmid,h,w]: the transposed convolution after its ELU
static ElScratch carve_expansion(Arena& a, int64_t B, int64_t Cmid, int64_t h, int64_t w) {
    ElScratch s;
    s.u = a.f((size_t)(B * Cmid * h * w));
    return s;
}

}  // namespace mcr
