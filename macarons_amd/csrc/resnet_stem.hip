// The front of the depth module's ResNet encoder (macarons/networks/ManyDepth.py:33-50 FeatureExtractor; DepthDecoder.forward runs it on
// the target image and again on the source images, :486-500), for BatchNorm in eval mode, fused, for gfx950 -- the forward.
//
//   z     = conv2d(x, weight [Cout,Cin,7,7], bias or none; stride 2, zero padding 3)      [N,Cout,Hc,Wc], Hc = (H-1)/2+1, Wc likewise
//   conv1 = max( fmaf(z + bias, a, b), 0 )                                                 a = bn_weight * (1.0f / sqrtf(var + eps)),
//                                                                                          b = fmaf(-mean, a, bn_bias), in float
//   pooled = max_pool2d(conv1, 3, stride 2, padding 1)                                    [N,Cout,Hp,Wp], Hp = (Hc-1)/2+1, Wp likewise;
//                                                                                          window cells outside the map are ignored
//
// ONE launch (resnet_stem_kernel) for the images of two operands, x [N0,..] and x_more [N1,..]: the target and the sources go through
// together without a concatenated copy; conv1 is stored for x's images only, and only where it is asked for.
//
// The tile.  A workgroup of four waves owns 2 x 15 pooled pixels (RS_PH x RS_PW) of one image and every output channel.  Their windows
// cover 5 rows x 31 columns of the convolution, from row 2 py0 - 1 and column 2 px0 - 1: the one-row, one-column halo above and left is
// recomputed (the tile to the right and below owns nothing of it); 32 columns are computed, two 16-pixel segments, the last one unused.
// Those need 15 rows x 69 columns of every input channel from (4 py0 - 5, 4 px0 - 5), staged once with zeros outside the image.  The
// products run on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain) as an implicit GEMM: K = Cin 49 in the weight's own
// order k = c 49 + di 7 + dj, padded with zeros to a multiple of 4 (zero weights times zeros, selected in place of the staged pixel a padded k
// would read: an Inf or NaN pixel stays within the windows that cover it); A is 16 output channels x 4 k, B is 4 k x 16 pixels of a
// convolution row, D 16 channels x 16 pixels.  Wave w owns output channels 16 w .. 16 w + 15 over the whole tile: 10 independent
// accumulators, one A read for ten products.  The weights pass through LDS 64 k at a time (RS_KCH), a channel's row 68 floats long
// (4 mod 32: the A reads of a wave, 16 channels x 4 k, fall on 64 distinct banks).  Why 2 x 15: every output channel has to sit in one
// workgroup for the input tile to be staged once, and the epilogue's tile [64][5 x 32] (41 KB) reuses the staging area (8 channels of
// input, 33 KB, and 17 KB of weights): 51 KB, three workgroups a compute unit; four pooled rows would need 73 KB for the epilogue alone.
// At 256 x 456 that is 32 x 8 workgroups an image, 768 for upstream's three images on 256 compute units.
//
// Stride 2.  Pixel p of a convolution row reads input column 2 p + dj: a wave's 16 B lanes would step two floats.  So even and odd
// columns are staged apart: input column j of a row lies at [j & 1][j >> 1], each half-row 35 floats, and tap dj reads half dj & 1 from
// dj >> 1 on, 16 consecutive floats per k, as in the stride-1 kernel.  The four k of one instruction are four consecutive taps, which
// start at 0, 35, 1, 36 (+ a row or a channel where the tap wraps): of 64 banks two pairs of 16-float windows overlap by 15, a two-way
// conflict on one B read in 32 cycles of matrix work -- left as it is.
//
// The epilogue applies bias, BatchNorm and ReLU to the accumulators and puts the tile in LDS; the workgroup then stores the 4 x 30 conv1
// pixels it owns (rows 2 py0 .. 2 py0 + 3, columns 2 px0 .. 2 px0 + 29) and pools out of LDS.  No atomics: two calls give the same bits.
//
// mcr_feature_extractor (below) is this launch followed by the basic blocks of basic_block.h on `pooled`.
#include "basic_block.h"

using namespace mcr;

namespace {

constexpr int RS_MAX_CIN = 8, RS_MAX_COUT = 64, RS_MAX_BLOCKS = 4;
constexpr int RS_PH = 2, RS_PW = 15;                                   // the pooled tile
constexpr int RS_CR = 2 * RS_PH + 1, RS_CW = 32;                       // the convolution rows and columns computed
constexpr int RS_IR = 2 * RS_CR + 5, RS_IC = 2 * RS_CW + 5;            // the input rows and columns staged (15 x 69)
constexpr int RS_QS = (RS_IC + 1) / 2, RS_ROW = 2 * RS_QS, RS_CH = RS_IR * RS_ROW;   // a half-row, a row, a channel of the staged input
constexpr int RS_KCH = 64, RS_KS = el_pad4(RS_KCH);                    // k per weight chunk, a channel's row of it
constexpr int RS_MAX_K = RS_MAX_CIN * 49;
constexpr int RS_OS = RS_CR * RS_CW + 4;                               // a channel of the epilogue's tile (4 mod 16: the four channel
                                                                       // groups of a store fall on distinct banks)
constexpr int RS_STAGE = RS_MAX_CIN * RS_CH + RS_MAX_COUT * RS_KS, RS_EPI = RS_MAX_COUT * RS_OS;
constexpr int RS_SM = RS_STAGE > RS_EPI ? RS_STAGE : RS_EPI;
static_assert(RS_MAX_K % 4 == 0 && RS_KCH % 4 == 0 && RS_MAX_COUT == 64, "whole k steps; a wave per 16 output channels");

struct StemBn { const float *weight, *bias, *mean, *var; float eps; };

// grid (N tiles), 256 threads; N = N0 + N1 images, image n from x for n < N0 and from x_more otherwise.
__global__ __launch_bounds__(256) void resnet_stem_kernel(const float* __restrict__ x, const float* __restrict__ x_more,
                                                          const float* __restrict__ weight, const float* __restrict__ cbias, StemBn bn,
                                                          float* __restrict__ pooled, float* __restrict__ conv1, int N0, int Cin, int Cout,
                                                          int H, int W, int Hc, int Wc, int Hp, int Wp, int tiles_x, int tiles) {
    constexpr int NT = 256;
    __shared__ float sm[RS_SM];
    __shared__ int koff[RS_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lk = lane >> 4, lp = lane & 15;
    const int tile = blockIdx.x % tiles, n = blockIdx.x / tiles;
    const int py0 = (tile / tiles_x) * RS_PH, px0 = (tile % tiles_x) * RS_PW;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;                    // the convolution tile's first row and column (-1 at the edge)
    const int iy0 = 4 * py0 - 5, ix0 = 4 * px0 - 5;                    // the staged input's
    const int K = Cin * 49, Kpad = (K + 3) & ~3, cob = (Cout + 15) >> 4;
    const size_t plane = (size_t)H * W;
    const float* img = n < N0 ? x + (size_t)n * Cin * plane : x_more + (size_t)(n - N0) * Cin * plane;
    float* wsm = sm + RS_MAX_CIN * RS_CH;

    for (int e = tid; e < Cin * RS_IR * RS_IC; e += NT) {
        const int c = e / (RS_IR * RS_IC), rem = e - c * (RS_IR * RS_IC);
        const int i = rem / RS_IC, j = rem - i * RS_IC;
        const int gy = iy0 + i, gx = ix0 + j;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float v = img[in ? (size_t)c * plane + (size_t)gy * W + gx : 0];
        sm[c * RS_CH + i * RS_ROW + (j & 1) * RS_QS + (j >> 1)] = in ? v : 0.f;
    }
    for (int k = tid; k < Kpad; k += NT) {                             // where tap k of pixel (row 0, column 0) lies; the padded tail
        const int c = k / 49, t = k - c * 49, di = t / 7, dj = t - di * 7;          // is given an address that exists and multiplies zeros
        koff[k] = k < K ? c * RS_CH + di * RS_ROW + (dj & 1) * RS_QS + (dj >> 1) : 0;
    }

    el_f32x4 acc[RS_CR * 2];
#pragma unroll
    for (int q = 0; q < RS_CR * 2; ++q) acc[q] = el_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kc0 = 0; kc0 < Kpad; kc0 += RS_KCH) {
        __syncthreads();                                               // the chunk before this one has been multiplied
        for (int e = tid; e < cob * 16 * RS_KCH; e += NT) {
            const int co = e / RS_KCH, kk = e - co * RS_KCH, k = kc0 + kk;
            const bool live = co < Cout && k < K;
            const float v = weight[live ? (size_t)co * K + k : 0];
            wsm[co * RS_KS + kk] = live ? v : 0.f;
        }
        __syncthreads();
        const int kn = min(RS_KCH, Kpad - kc0);
        if (wave < cob) {
            const float* ab = wsm + (wave * 16 + lp) * RS_KS + lk;
            for (int s = 0; s < kn; s += 4) {
                const float a = ab[s];
                const bool live = kc0 + s + lk < K;                    // a padded k multiplies 0 by 0, whatever the tile holds
                const float* xb = sm + koff[kc0 + s + lk] + lp;
#pragma unroll
                for (int r = 0; r < RS_CR; ++r)
#pragma unroll
                    for (int g = 0; g < 2; ++g)
                        acc[r * 2 + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, live ? xb[r * 2 * RS_ROW + g * 16] : 0.f, acc[r * 2 + g], 0, 0, 0);
            }
        }
    }

    // Element j of lane l of accumulator (r, g) is output channel 16 wave + (l >> 4) 4 + j at convolution pixel (row r, column
    // 16 g + (l & 15)) of the tile.
    __syncthreads();
    if (wave < cob) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = wave * 16 + lk * 4 + j;
            if (co < Cout) {
                const float a = bn.weight[co] * (1.0f / sqrtf(bn.var[co] + bn.eps));
                const float b = fmaf(-bn.mean[co], a, bn.bias[co]);
                const float cb = cbias ? cbias[co] : 0.f;
#pragma unroll
                for (int r = 0; r < RS_CR; ++r)
#pragma unroll
                    for (int g = 0; g < 2; ++g) sm[co * RS_OS + r * RS_CW + g * 16 + lp] = fmaxf(fmaf(acc[r * 2 + g][j] + cb, a, b), 0.f);
            }
        }
    }
    __syncthreads();

    if (conv1 != nullptr && n < N0) {
        constexpr int OR = 2 * RS_PH, OC = 2 * RS_PW;                  // the convolution pixels this tile owns, from tile cell (1, 1)
        float* ob = conv1 + (size_t)n * Cout * Hc * Wc;
        for (int o = tid; o < Cout * OR * OC; o += NT) {
            const int co = o / (OR * OC), rem = o - co * (OR * OC);
            const int ty = 1 + rem / OC, tx = 1 + rem % OC;
            const int cy = cy0 + ty, cx = cx0 + tx;
            if (cy < Hc && cx < Wc) ob[((size_t)co * Hc + cy) * Wc + cx] = sm[co * RS_OS + ty * RS_CW + tx];
        }
    }
    float* pb = pooled + (size_t)n * Cout * Hp * Wp;
    for (int o = tid; o < Cout * RS_PH * RS_PW; o += NT) {
        const int co = o / (RS_PH * RS_PW), rem = o - co * (RS_PH * RS_PW);
        const int ly = rem / RS_PW, lx = rem - ly * RS_PW;
        const int py = py0 + ly, px = px0 + lx;
        if (py >= Hp || px >= Wp) continue;
        float m = -INFINITY;                                           // the window's centre is always inside the map
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ty = 2 * ly + dy, tx = 2 * lx + dx;
                const int cy = cy0 + ty, cx = cx0 + tx;
                if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) m = fmaxf(m, sm[co * RS_OS + ty * RS_CW + tx]);
            }
        pb[((size_t)co * Hp + py) * Wp + px] = m;
    }
}

struct StemSizes { int Hc, Wc, Hp, Wp; };
StemSizes stem_sizes(int64_t H, int64_t W) {
    StemSizes s;
    s.Hc = (int)((H - 1) / 2 + 1), s.Wc = (int)((W - 1) / 2 + 1);
    s.Hp = (s.Hc - 1) / 2 + 1, s.Wp = (s.Wc - 1) / 2 + 1;
    return s;
}

bool stem_sizes_ok(int64_t N0, int64_t N1, int64_t Cin, int64_t Cout, int64_t H, int64_t W) {
    if (N0 < 0 || N1 < 0 || N0 > 0x7fffffffll || N1 > 0x7fffffffll || N0 + N1 < 1) return false;
    if (Cin < 1 || Cin > RS_MAX_CIN || Cout < 1 || Cout > RS_MAX_COUT || H < 1 || W < 1 || H > 0x7fffffffll || W > 0x7fffffffll) return false;
    const StemSizes s = stem_sizes(H, W);
    return el_fits(N0 + N1, Cin, H, W) && el_fits(N0 + N1, Cout, s.Hc, s.Wc);      // the largest of x, x_more, conv1 and pooled
}

int stem_check(const char* who, const float* x, const float* x_more, const float* weight, const StemBn& bn, const float* pooled, int64_t N0,
               int64_t N1, int Cin, int Cout, int H, int W) {
    MCR_REQUIRE(H >= 1 && W >= 1, "%s: the images are %d x %d, H and W must be at least 1", who, H, W);
    MCR_REQUIRE(Cin >= 1 && Cin <= RS_MAX_CIN && Cout >= 1 && Cout <= RS_MAX_COUT,
                "%s: Cin = %d, Cout = %d channels, Cin 1 .. %d and Cout 1 .. %d are supported", who, Cin, Cout, RS_MAX_CIN, RS_MAX_COUT);
    MCR_REQUIRE(N0 >= 0 && N1 >= 0 && N0 + N1 >= 1, "%s: N0 = %lld and N1 = %lld images, neither may be negative and N0 + N1 must be at least 1",
                who, (long long)N0, (long long)N1);
    MCR_REQUIRE(stem_sizes_ok(N0, N1, Cin, Cout, H, W), "%s: N0 + N1 = %lld + %lld, channels %d -> %d, %d x %d: a tensor has 2^31 elements or more",
                who, (long long)N0, (long long)N1, Cin, Cout, H, W);
    MCR_REQUIRE((N0 == 0 || x) && (N1 == 0 || x_more) && weight && bn.weight && bn.bias && bn.mean && bn.var && pooled, "%s: NULL operand", who);
    return 0;
}

void stem_launch(hipStream_t st, const float* x, const float* x_more, const float* weight, const float* cbias, const StemBn& bn, float* pooled,
                 float* conv1, int64_t N0, int64_t N1, int Cin, int Cout, int H, int W) {
    const StemSizes s = stem_sizes(H, W);
    const int tx = (int)cdiv(s.Wp, RS_PW), tiles = tx * (int)cdiv(s.Hp, RS_PH);
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)((N0 + N1) * tiles)), dim3(256), 0, st, x, x_more, weight, cbias, bn, pooled,
                       N0 ? conv1 : nullptr, (int)N0, Cin, Cout, H, W, s.Hc, s.Wc, s.Hp, s.Wp, tx, tiles);
}

// The extractor's scratch: the first convolution of a block, and the map the blocks alternate with `features` (block i reads one and
// writes the other, so that the last one writes `features`).
struct ExtractorScratch { float *t, *other; };
ExtractorScratch carve_extractor(Arena& a, int64_t N, int64_t Cout, int64_t Hp, int64_t Wp, int n_blocks) {
    ExtractorScratch s{nullptr, nullptr};
    if (n_blocks > 0) {
        s.t = carve_block(a, N, Cout, Hp, Wp).t;
        s.other = a.f((size_t)(N * Cout * Hp * Wp));
    }
    return s;
}

}  // namespace

extern "C" int mcr_resnet_stem(const float* x, const float* x_more, const float* weight, const float* bias, const float* bn_weight,
                               const float* bn_bias, const float* bn_mean, const float* bn_var, float eps, float* pooled, float* conv1,
                               int64_t N0, int64_t N1, int Cin, int Cout, int H, int W, void* stream) {
    const char* who = "mcr_resnet_stem";
    const StemBn bn{bn_weight, bn_bias, bn_mean, bn_var, eps};
    if (int e = stem_check(who, x, x_more, weight, bn, pooled, N0, N1, Cin, Cout, H, W)) return e;
    stem_launch((hipStream_t)stream, x, x_more, weight, bias, bn, pooled, conv1, N0, N1, Cin, Cout, H, W);
    MCR_LAUNCH_CHECK("resnet_stem_kernel");
    return 0;
}

extern "C" size_t mcr_feature_extractor_workspace_bytes(int64_t N0, int64_t N1, int64_t Cin, int64_t Cout, int64_t H, int64_t W,
                                                        int64_t n_blocks) {
    if (!stem_sizes_ok(N0, N1, Cin, Cout, H, W) || n_blocks < 0 || n_blocks > RS_MAX_BLOCKS) return 0;
    const StemSizes s = stem_sizes(H, W);
    return measure(carve_extractor, N0 + N1, Cout, (int64_t)s.Hp, (int64_t)s.Wp, (int)n_blocks);
}

extern "C" int mcr_feature_extractor(const float* x, const float* x_more, const float* weight, const float* bias, const float* bn_weight,
                                     const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                                     const float* const* block_pointers, const float* block_eps, int n_blocks, float* features, float* conv1,
                                     int64_t N0, int64_t N1, int Cin, int Cout, int H, int W, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const char* who = "mcr_feature_extractor";
    const StemBn bn{bn_weight, bn_bias, bn_mean, bn_var, eps};
    if (int e = stem_check(who, x, x_more, weight, bn, features, N0, N1, Cin, Cout, H, W)) return e;
    MCR_REQUIRE(n_blocks >= 0 && n_blocks <= RS_MAX_BLOCKS, "%s: n_blocks = %d, 0 .. %d are supported", who, n_blocks, RS_MAX_BLOCKS);
    MCR_REQUIRE(n_blocks == 0 || (block_pointers && block_eps), "%s: NULL operand", who);
    for (int i = 0; i < n_blocks; ++i) MCR_REQUIRE(block_operands(block_pointers + 10 * i, block_eps + 2 * i).all(), "%s: NULL operand", who);
    const StemSizes s = stem_sizes(H, W);
    const int64_t N = N0 + N1;
    // (without blocks nothing is needed and nothing is asked for: a NULL workspace is accepted where the size function says 0 bytes)
    if (n_blocks > 0)
        if (int e = check_workspace(who, workspace, workspace_bytes, mcr_feature_extractor_workspace_bytes(N0, N1, Cin, Cout, H, W, n_blocks))) return e;
    Arena arena{(char*)workspace, workspace_bytes};
    const ExtractorScratch ws = carve_extractor(arena, N, Cout, s.Hp, s.Wp, n_blocks);
    const hipStream_t st = (hipStream_t)stream;
    float* cur = n_blocks % 2 ? ws.other : features;
    stem_launch(st, x, x_more, weight, bias, bn, cur, conv1, N0, N1, Cin, Cout, H, W);
    MCR_LAUNCH_CHECK("resnet_stem_kernel");
    for (int i = 0; i < n_blocks; ++i) {
        float* next = cur == features ? ws.other : features;
        bb_launch(st, cur, block_operands(block_pointers + 10 * i, block_eps + 2 * i), ws.t, next, N, Cout, s.Hp, s.Wp);
        MCR_LAUNCH_CHECK("el_conv_kernel (basic block)");
        cur = next;
    }
    return 0;
}
