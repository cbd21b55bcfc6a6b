// The expansion layers of the depth decoder (macarons/networks/ManyDepth.py:308-363 ExpansionLayer; expansion5..1 of the decoder, :428-471
// and :514-529), fused, for gfx950 -- the forward.
//
//   u = ELU( conv_transpose2d(x, Wu[Cin,Cmid,3,3], bu; stride 1, padding 1) )      [B,Cmid,h,w]
//   r = nearest(u -> (H,W))                                                         torch's mode='nearest': source = min(floor(dst in/out), in-1), in float
//   c = cat(r, x_add) over channels                                                 x_add [B,Cadd,H,W], or absent (Cadd = 0)
//   y = ELU( conv2d(reflect_pad1(c), Wi[Cout,Cmid+Cadd,3,3], bi) )                  [B,Cout,H,W]
//
// Two launches of ONE kernel template, el_conv_kernel: a 3 x 3 correlation over a virtual input of C0 + C1 channels, bias, ELU.  The first
// launch reads the transposed convolution as what it is, a zero-padded correlation with the kernel flipped and its channel axes
// exchanged (tap (di,dj) of output channel co and input channel ci is Wu[ci,co,2-di,2-dj]), over x, into the workspace.  The second reads
// channels below Cmid from u through the nearest-source index and the others from x_add, both through the reflection index: no
// resized, concatenated or padded tensor exists.  What differs between the two is a table of source offsets per cell of the staged region
// (-1: a zero) that the workgroup builds once, and the order in which the weights are read.
//
// The products run on v_mfma_f32_16x16x4_f32, exact fp32 (a k-ordered fmaf chain), as an implicit GEMM per tap: the A operand is 16 output
// channels x 4 input channels of one tap, the B operand 4 input channels x 16 consecutive pixels of a row of the LDS tile, shifted by the
// tap; D is 16 output channels x 16 pixels.  A workgroup of four waves owns TH rows x 16 NSEG columns of one image and 16 MA output
// channels.  KC input channels at a time the tile with its one-pixel ring and the weights of those channels go to LDS -- the weights in
// upstream's own layouts, rearranged to [output channel][channel][tap] (the transposed convolution's taps flipped) while they are staged,
// so nothing is cached on the host; an output channel's row is 2 mod 32 floats long, which keeps the A reads of a wave on distinct banks (9 is
// odd) and the stores of the convolution's weights lane-linear -- through registers, the next chunk on its way while this one is multiplied.  The four waves divide the rows (WK = 1), or, where the map is so
// small that this would leave compute units idle, the input channels of every chunk (WK = 4: groups of four channels round-robin); every
// wave keeps at least two independent accumulators.  The partial sums of a split are added through LDS in the order of the waves, then
// the bias, then ELU: no atomics, two calls give the same bits.
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

// grid (B co_blocks tiles), 256 threads.  src0 [B,C0,h0,w0] and src1 [B,C1,H,W] (C1 = 0: absent) are the virtual input's channels
// 0 .. C0-1 and C0 .. C0+C1-1; out [B,Cout,H,W].  UP: the transposed convolution's launch (h0 x w0 = H x W, zero padding, weight
// [C0,Cout,3,3] flipped); otherwise the convolution's (reflection, src0 through the nearest index with scales sy = h0 / H, sx = w0 / W,
// weight [Cout,C0+C1,3,3]).
template <bool UP, int TH, int NSEG, int MA, int WK, int KC>
__global__ __launch_bounds__(256) void el_conv_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                      const float* __restrict__ weight, const float* __restrict__ bias, float* __restrict__ out,
                                                      int C0, int C1, int h0, int w0, int Cout, int H, int W, float sy, float sx, int tiles_x,
                                                      int tiles, int co_blocks) {
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

    // cell r = ry RW + rx of the region is the padded coordinate (y0 - 1 + ry, x0 - 1 + rx): where it comes from in a plane of src0 and
    // of src1, -1 for a zero (the zero ring of the transposed convolution; a coordinate past the mirror, which no pixel of the image reads)
    for (int r = tid; r < R; r += NT) {
        const int ry = r / RW, rx = r - ry * RW;
        const int cy = y0 - 1 + ry, cx = x0 - 1 + rx;              // >= -1
        int o0 = -1, o1 = -1;
        if (UP) {
            if (cy >= 0 && cy < H && cx >= 0 && cx < W) o0 = cy * w0 + cx;
        } else if (cy <= H && cx <= W) {
            const int my = el_reflect(cy, H), mx = el_reflect(cx, W);
            o1 = my * W + mx;
            o0 = el_nearest(my, sy, h0) * w0 + el_nearest(mx, sx, w0);
        }
        off0[r] = o0, off1[r] = o1;
    }
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
        if (co0 + co < Cout && i < H && jx < W) ob[(size_t)(co0 + co) * plane1 + (size_t)i * W + jx] = el_elu(z + bias[co0 + co]);
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

template <bool UP, int TH, int NSEG, int MA, int WK, int KC>
static void el_launch_as(hipStream_t st, const float* src0, const float* src1, const float* weight, const float* bias, float* out, int64_t B,
                         int C0, int C1, int h0, int w0, int Cout, int H, int W) {
    const int tx = (int)cdiv(W, 16 * NSEG), tiles = tx * (int)cdiv(H, TH), cob = (int)cdiv(Cout, 16 * MA);
    hipLaunchKernelGGL((el_conv_kernel<UP, TH, NSEG, MA, WK, KC>), dim3((unsigned)(B * cob * tiles)), dim3(256), 0, st, src0, src1, weight, bias,
                       out, C0, C1, h0, w0, Cout, H, W, (float)h0 / (float)H, (float)w0 / (float)W, tx, tiles, cob);
}

template <bool UP>
static void el_launch(hipStream_t st, const float* src0, const float* src1, const float* weight, const float* bias, float* out, int64_t B, int C0,
                      int C1, int h0, int w0, int Cout, int H, int W) {
    switch (el_tile(B, Cout, H, W)) {
        case EL_ROWS16: el_launch_as<UP, 4, 2, 1, 1, 16>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
        case EL_ROWS32: el_launch_as<UP, 4, 2, 2, 1, 16>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
        case EL_SPLIT: el_launch_as<UP, 2, 1, 1, 4, 32>(st, src0, src1, weight, bias, out, B, C0, C1, h0, w0, Cout, H, W); break;
    }
}

static bool el_fits(int64_t B, int64_t C, int64_t H, int64_t W) { return H * W <= 0x7fffffffll && B <= 0x7fffffffll / (C * H * W); }

static bool el_sizes_ok(int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h, int64_t w, int64_t H, int64_t W) {
    if (B < 1 || Cin < 1 || Cin > EL_MAX_C || Cmid < 1 || Cmid > EL_MAX_C || Cout < 1 || Cout > EL_MAX_C) return false;
    if (Cadd < 0 || Cmid + Cadd > EL_MAX_C || h < 1 || w < 1 || H < 2 || W < 2) return false;
    if (h > 0x7fffffffll || w > 0x7fffffffll || H > 0x7fffffffll || W > 0x7fffffffll) return false;
    return el_fits(B, Cin, h, w) && el_fits(B, Cmid, h, w) && el_fits(B, Cout, H, W) && (Cadd == 0 || el_fits(B, Cadd, H, W));
}

struct ElScratch { float* u; };                        // [B,Cmid,h,w]: the transposed convolution after its ELU
static ElScratch carve_expansion(Arena& a, int64_t B, int64_t Cmid, int64_t h, int64_t w) {
    ElScratch s;
    s.u = a.f((size_t)(B * Cmid * h * w));
    return s;
}

}  // namespace mcr

using namespace mcr;

extern "C" size_t mcr_expansion_layer_workspace_bytes(int64_t B, int64_t Cmid, int64_t h, int64_t w) {
    if (B < 1 || Cmid < 1 || Cmid > EL_MAX_C || h < 1 || w < 1 || h > 0x7fffffffll || w > 0x7fffffffll || !el_fits(B, Cmid, h, w)) return 0;
    return measure(carve_expansion, B, Cmid, h, w);
}

extern "C" int mcr_expansion_layer(const float* x, const float* x_add, const float* up_weight, const float* up_bias, const float* i_weight,
                                   const float* i_bias, float* y, int64_t B, int Cin, int Cmid, int Cadd, int Cout, int h, int w, int H, int W,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_expansion_layer";
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
    MCR_REQUIRE(x && up_weight && up_bias && i_weight && i_bias && y && (Cadd == 0 || x_add), "%s: NULL operand", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_expansion_layer_workspace_bytes(B, Cmid, h, w))) return e;
    Arena arena{(char*)workspace, workspace_bytes};
    const ElScratch ws = carve_expansion(arena, B, Cmid, h, w);
    const hipStream_t st = (hipStream_t)stream;
    el_launch<true>(st, x, nullptr, up_weight, up_bias, ws.u, B, Cin, 0, h, w, Cmid, h, w);
    MCR_LAUNCH_CHECK("el_conv_kernel (transposed convolution)");
    el_launch<false>(st, ws.u, Cadd ? x_add : nullptr, i_weight, i_bias, y, B, Cmid, Cadd, h, w, Cout, H, W);
    MCR_LAUNCH_CHECK("el_conv_kernel (convolution)");
    return 0;
}
