// Backward of the plane sweep of the depth module (cost_volume.hip) for gfx950: gradients of the target features x and of the source
// features x_alpha; the cameras and the bins are constants.  With g = d loss / d cv and s_c(k,p) = sign(m_c - x_c) in {-1, 0, +1}:
//   d_x[b,c,p]           = -(1/C)   sum_k g[b,k,p] s_c(k,p)
//   d_x_alpha[b,a,c,y,x] = 1/(A C)  sum over the (k, p, corner) that land on (y, x) of  w_corner g[b,k,p] s_c(k,p)
// No intermediate has a channel axis per (source, plane, position): the only channel data per (plane, position) is the sign state, 2 bits a
// channel (16 bytes).  No floating-point atomics: two runs give the same bits.
//
// Passes (d_x_alpha = NULL leaves out 4..8, d_x = NULL leaves out 3):
//   0. cv_maxabs_kernel        max |g| as an integer maximum of the bit patterns (a pattern of 0x7f800000 or more: g is not finite)
//   1. cv_channels_last_kernel the forward's layout pass (cost_volume.hip)
//   2. cv_sign_sweep_kernel    the forward's sweep (cv_sweep_row, cost_volume.h: the same instructions), which keeps per (b,k,p) and lane one
//                              byte, bits 0..3 = m_c - x_c != 0 and bits 4..7 = m_c - x_c < 0 of its four channels, and per (b,a,k,p) the
//                              pixel coordinate it sampled at
//   3. cv_dx_kernel            one row of 16 lanes per (b,p): sum over the planes, ascending
//   4. cv_scatter_kernel<0>    counts the non-zero corners per destination pixel (b,a,y,x)          (integer atomics)
//   5. cv_scan_kernel          exclusive scan of the counts: the list of a destination is [off[n], off[n+1])
//   6. cv_scatter_kernel<1>    fills the lists with (k*P + p, w_corner * g) through an integer cursor -- the order inside a list is whatever
//                              the cursor gave
//   7. cv_dest_sum_kernel      one wave per destination (four rows of 16 lanes, every fourth entry each) walks its list and adds q = llrint(w g 2^32 / max|g|), negated or not
//                              or not at all per channel, in 64-bit integers: exact, so the order does not matter.  |q| <= 2^32 and a list
//                              has fewer than 2^31 entries, so the sum stays inside 63 bits; an entry is quantised to 2^-33 of max|g|.
//                              Writes a channels-last gradient over the forward's channels-last copy, which is dead by then.
//   8. cv_from_channels_last_kernel   back to [B,A,C,Hf,Wf] through LDS.
// max|g| = 0 gives two zero gradients (every product is 0); a g that is not finite gives two gradients of NaN.
#include "cost_volume.h"

namespace mcr {

constexpr unsigned CV_INF_BITS = 0x7f800000u;
constexpr int CV_SCAN_THREADS = 1024;

__global__ __launch_bounds__(256) void cv_maxabs_kernel(const float* __restrict__ g, int64_t batch_stride, int64_t per_batch,
                                                        unsigned* __restrict__ maxbits) {
    unsigned m = 0;
    const float* gb = g + (size_t)blockIdx.y * batch_stride;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < per_batch; t += (int64_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(fabsf(gb[t])));                          // NaN patterns lie above infinity's
    m = wave_max_all(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxbits, m);
}

__global__ __launch_bounds__(256) void cv_sign_sweep_kernel(const float* __restrict__ x, const float* __restrict__ xa_cl,
                                                            const double* __restrict__ pose, const float* __restrict__ bins,
                                                            unsigned char* __restrict__ masks, float2* __restrict__ samples, int A, int H, int W,
                                                            int Hf, int Wf, int D, float fov_scale) {
    const int lane = threadIdx.x & 15;
    const int P = Hf * Wf;
    const int pos_raw = blockIdx.x * CV_POS + (threadIdx.x >> 4);
    const bool valid = pos_raw < P;
    const int pos = valid ? pos_raw : P - 1;
    const int b = blockIdx.z;
    const int k0 = blockIdx.y * CV_PLANES;
    float4 acc[CV_PLANES];
    if (samples)
        cv_sweep_row<true>(xa_cl, pose, bins, samples, b, k0, pos, valid, lane, A, H, W, Hf, Wf, D, fov_scale, acc);
    else
        cv_sweep_row<false>(xa_cl, pose, bins, nullptr, b, k0, pos, valid, lane, A, H, W, Hf, Wf, D, fov_scale, acc);

    const float* xt = x + ((size_t)b * CV_C + lane * 4) * (size_t)P + pos;
    const float x0v = xt[0], x1v = xt[P], x2v = xt[2 * (size_t)P], x3v = xt[3 * (size_t)P];
    const float inv_a = 1.f / (float)A;
#pragma unroll
    for (int kk = 0; kk < CV_PLANES; ++kk) {
        const float d0 = acc[kk].x * inv_a - x0v, d1 = acc[kk].y * inv_a - x1v, d2 = acc[kk].z * inv_a - x2v, d3 = acc[kk].w * inv_a - x3v;
        const unsigned bits = (d0 != 0.f ? 1u : 0u) | (d1 != 0.f ? 2u : 0u) | (d2 != 0.f ? 4u : 0u) | (d3 != 0.f ? 8u : 0u) |
                              (d0 < 0.f ? 16u : 0u) | (d1 < 0.f ? 32u : 0u) | (d2 < 0.f ? 64u : 0u) | (d3 < 0.f ? 128u : 0u);
        if (valid && k0 + kk < D) masks[(((size_t)b * D + (k0 + kk)) * (size_t)P + pos) * 16 + lane] = (unsigned char)bits;
    }
}

// +v, -v or 0 by the sign state of channel ch (0..3) of a lane's byte.
template <typename T>
__device__ __forceinline__ T cv_signed(unsigned bits, int ch, T v) {
    return (bits >> ch) & 1u ? ((bits >> (4 + ch)) & 1u ? -v : v) : (T)0;
}

__global__ __launch_bounds__(256) void cv_dx_kernel(const float* __restrict__ g, int64_t g_batch_stride, const unsigned char* __restrict__ masks,
                                                    const unsigned* __restrict__ maxbits, float* __restrict__ d_x, int P, int D) {
    const int lane = threadIdx.x & 15;
    const int pos = blockIdx.x * CV_POS + (threadIdx.x >> 4);
    const int b = blockIdx.y;
    if (pos >= P) return;
    const float* gp = g + (size_t)b * g_batch_stride + pos;
    const unsigned char* mp = masks + ((size_t)b * D * (size_t)P + pos) * 16 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < D; ++k) {                                          // ascending: a fixed order
        const float gk = gp[(size_t)k * P];
        const unsigned bits = mp[(size_t)k * P * 16];
        a0 += cv_signed(bits, 0, gk), a1 += cv_signed(bits, 1, gk), a2 += cv_signed(bits, 2, gk), a3 += cv_signed(bits, 3, gk);
    }
    const bool bad = *maxbits >= CV_INF_BITS;
    const float sc = -1.f / CV_C;
    float* o = d_x + ((size_t)b * CV_C + lane * 4) * (size_t)P + pos;
    o[0] = bad ? NAN : a0 * sc, o[P] = bad ? NAN : a1 * sc, o[2 * (size_t)P] = bad ? NAN : a2 * sc, o[3 * (size_t)P] = bad ? NAN : a3 * sc;
}

// One thread per sample (b,a,k,p).  FILL = false: counts[dest] += 1 for every corner of non-zero weight.  FILL = true: the same corners, by
// the same test on the same bits, take a slot of their destination's list each.
template <bool FILL>
__global__ __launch_bounds__(256) void cv_scatter_kernel(const float2* __restrict__ samples, const float* __restrict__ g, int64_t g_batch_stride,
                                                         unsigned* __restrict__ counts_or_cursor, const unsigned* __restrict__ off,
                                                         int2* __restrict__ entries, int64_t n_samples, int A, int Hf, int Wf, int D) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_samples) return;
    const int P = Hf * Wf;
    const int64_t bak = t / P;
    const int p = (int)(t - bak * P);
    const int64_t ba = bak / D;
    const int k = (int)(bak - ba * D);
    const float2 smp = samples[t];
    const bool in = smp.x > -1.5f;                                         // CV_NOT_IN is -2, a sampled coordinate is above -1
    if (!in) return;
    const CvCorners cn = cv_corners(smp.x, smp.y, true, Hf, Wf);
    const int pix[4] = {cn.y0c * Wf + cn.x0c, cn.y0c * Wf + cn.x1c, cn.y1c * Wf + cn.x0c, cn.y1c * Wf + cn.x1c};
    const float w[4] = {cn.w00, cn.w01, cn.w10, cn.w11};
    const float gk = FILL ? g[(ba / A) * g_batch_stride + (int64_t)k * P + p] : 0.f;
#pragma unroll
    for (int cnr = 0; cnr < 4; ++cnr) {
        if (w[cnr] != 0.f) {
            const int64_t dest = ba * P + pix[cnr];
            const unsigned slot = atomicAdd(counts_or_cursor + dest, 1u);
            if (FILL) {
                if (slot < off[dest + 1]) entries[slot] = make_int2(k * P + p, __float_as_int(w[cnr] * gk));   // never false: the same test counted
            }
        }
    }
}

// In place: counts[0..n) -> exclusive offsets, counts[n] = the total; cursor[j] = offset j.  One workgroup; thread i owns a contiguous chunk.
__global__ __launch_bounds__(CV_SCAN_THREADS) void cv_scan_kernel(unsigned* __restrict__ counts, unsigned* __restrict__ cursor, int64_t n) {
    __shared__ unsigned s_wave[CV_SCAN_THREADS / 64];
    const int64_t per = (n + CV_SCAN_THREADS - 1) / CV_SCAN_THREADS;
    const int64_t j0 = min(n, (int64_t)threadIdx.x * per), j1 = min(n, j0 + per);
    unsigned s = 0;
    for (int64_t j = j0; j < j1; ++j) s += counts[j];
    unsigned total;
    unsigned run = block_exclusive_scan<CV_SCAN_THREADS / 64>(s, s_wave, &total);      // of the chunk totals
    for (int64_t j = j0; j < j1; ++j) {
        const unsigned c = counts[j];
        counts[j] = run;
        cursor[j] = run;
        run += c;
    }
    if (threadIdx.x == CV_SCAN_THREADS - 1) counts[n] = total;
}

// A wave per destination: its four rows take every fourth entry of the list, lane l of each row channels 4l .. 4l+3, and the rows' integer
// sums are added across the wave -- exact in any order.
constexpr int CV_DEST_PER_WG = 4;

__global__ __launch_bounds__(256) void cv_dest_sum_kernel(const unsigned* __restrict__ off, const int2* __restrict__ entries,
                                                          const unsigned char* __restrict__ masks, const unsigned* __restrict__ maxbits,
                                                          float* __restrict__ d_cl, int64_t n_dest, int A, int P, int D) {
    const int lane = threadIdx.x & 15, sub = (threadIdx.x >> 4) & 3;
    const int64_t n = (int64_t)blockIdx.x * CV_DEST_PER_WG + (threadIdx.x >> 6);
    if (n >= n_dest) return;                                               // wave-uniform
    const unsigned mb = *maxbits;
    const bool bad = mb >= CV_INF_BITS;
    const double gmax = (double)__uint_as_float(mb);
    const double scale = (bad || mb == 0u) ? 0.0 : 4294967296.0 / gmax;
    const unsigned char* mp = masks + (size_t)(n / ((int64_t)A * P)) * D * (size_t)P * 16 + lane;
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    const unsigned e0 = off[n], e1 = off[n + 1];
    if (!bad) {
#pragma unroll 4
        for (unsigned e = e0 + sub; e < e1; e += 4) {
            const int2 ent = entries[e];
            const unsigned bits = mp[(size_t)ent.x * 16];
            const long long q = llrint((double)__int_as_float(ent.y) * scale);
            a0 += cv_signed(bits, 0, q), a1 += cv_signed(bits, 1, q), a2 += cv_signed(bits, 2, q), a3 += cv_signed(bits, 3, q);
        }
    }
    a0 = lanes_reduce<16, 32>(a0, op_add{}), a1 = lanes_reduce<16, 32>(a1, op_add{});        // the wave's four rows
    a2 = lanes_reduce<16, 32>(a2, op_add{}), a3 = lanes_reduce<16, 32>(a3, op_add{});
    if (sub) return;
    const double back = gmax * (1.0 / 4294967296.0) / ((double)A * CV_C);
    float4 o;
    o.x = bad ? NAN : (float)((double)a0 * back), o.y = bad ? NAN : (float)((double)a1 * back);
    o.z = bad ? NAN : (float)((double)a2 * back), o.w = bad ? NAN : (float)((double)a3 * back);
    *(float4*)(d_cl + (size_t)n * CV_C + lane * 4) = o;
}

// [img, P, 64] -> [img, 64, P]: the mirror of cv_channels_last_kernel.
__global__ __launch_bounds__(256) void cv_from_channels_last_kernel(const float* __restrict__ src, float* __restrict__ dst, int P) {
    __shared__ float tile[CV_C][CV_C + 1];
    const int64_t img = blockIdx.y;
    const int p0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int pp = ty; pp < 64; pp += 4) {
        const int p = p0 + pp;
        tile[tx][pp] = p < P ? src[(img * P + p) * CV_C + tx] : 0.f;
    }
    __syncthreads();
    for (int c = ty; c < CV_C; c += 4) {
        const int p = p0 + tx;
        if (p < P) dst[(img * CV_C + c) * P + p] = tile[c][tx];
    }
}

// The workspace.  counts and maxbits stay adjacent: the entry zeroes them with one memset.
struct CvBwdScratch {
    float* xa_cl;                                    // the source maps channels-last, later their gradient
    double* pose;
    unsigned char* masks;                            // the sign states
    float2* samples;
    unsigned *counts, *maxbits, *cursor;             // counts [n_dest + 1], then offsets
    int2* entries;                                   // room for four corners of every sample
};

static CvBwdScratch carve_cv_bwd(Arena& a, int64_t B, int64_t A, int64_t Hf, int64_t Wf, int64_t D) {
    const size_t P = (size_t)Hf * Wf, n_dest = (size_t)B * A * P, n_samples = n_dest * D;
    CvBwdScratch w;
    w.xa_cl = a.f(n_dest * CV_C);
    w.pose = (double*)a.bytes((size_t)B * A * 12 * sizeof(double));
    w.masks = (unsigned char*)a.bytes((size_t)B * D * P * 16);
    w.samples = (float2*)a.bytes(n_samples * sizeof(float2));
    w.counts = (unsigned*)a.bytes((n_dest + 1) * sizeof(unsigned));
    w.maxbits = (unsigned*)a.bytes(sizeof(unsigned));
    w.cursor = (unsigned*)a.bytes(n_dest * sizeof(unsigned));
    w.entries = (int2*)a.bytes(4 * n_samples * sizeof(int2));
    return w;
}

}  // namespace mcr

using namespace mcr;

extern "C" size_t mcr_cost_volume_backward_workspace_bytes(int64_t B, int64_t A, int64_t C, int64_t Hf, int64_t Wf, int64_t D) {
    if (B <= 0 || A <= 0 || C <= 0 || Hf <= 0 || Wf <= 0 || D <= 0) return 0;
    if (4.0 * (double)B * (double)A * (double)D * (double)Hf * (double)Wf > 2147483647.0) return 0;   // refused by the entry
    return measure(carve_cv_bwd, B, A, Hf, Wf, D);
}

extern "C" int mcr_cost_volume_backward(const float* x, const float* x_alpha, const float* cams, const float* depth_bins, const float* d_out,
                                        int64_t d_out_batch_stride, float* d_x, float* d_x_alpha, int64_t B, int A, int C, int H, int W, int Hf,
                                        int Wf, int D, float fov_scale, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_cost_volume_backward";
    if (int e = cv_check(who, x, x_alpha, cams, depth_bins, d_out, "d_out_batch_stride", d_out_batch_stride, B, A, C, H, W, Hf, Wf, D, fov_scale))
        return e;
    MCR_REQUIRE(d_x || d_x_alpha, "%s: nothing to do, d_x and d_x_alpha are both NULL", who);
    MCR_REQUIRE(4.0 * (double)B * A * D * Hf * Wf <= 2147483647.0,
                "%s: 4*B*A*D*Hf*Wf = %.0f corner contributions exceed the 2^31 - 1 that the lists index", who, 4.0 * (double)B * A * D * Hf * Wf);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_cost_volume_backward_workspace_bytes(B, A, C, Hf, Wf, D))) return e;

    const hipStream_t st = (hipStream_t)stream;
    const int P = Hf * Wf;
    Arena arena{(char*)workspace, workspace_bytes};
    const CvBwdScratch ws = carve_cv_bwd(arena, B, A, Hf, Wf, D);
    float2* samples = d_x_alpha ? ws.samples : nullptr;
    const int64_t n_dest = B * A * P, n_samples = n_dest * D, per_batch = (int64_t)D * P;

    // one memset for counts and maxbits: the carve hands them out back to back, so the span is the distance between the carved pointers
    // (whatever the rounding), not a sum of sizes written a second time
    if (int e = check_hip(hipMemsetAsync(ws.counts, 0, (char*)ws.cursor - (char*)ws.counts, st), "hipMemsetAsync(counts, maxbits)"))
        return e;
    hipLaunchKernelGGL(cv_maxabs_kernel, dim3((unsigned)min((int64_t)256, cdiv(per_batch, 256)), (unsigned)B), dim3(256), 0, st, d_out,
                       d_out_batch_stride, per_batch, ws.maxbits);
    MCR_LAUNCH_CHECK("cv_maxabs_kernel");
    cv_launch_channels_last(x_alpha, ws.xa_cl, P, cams, B, A, ws.pose, st);
    MCR_LAUNCH_CHECK("cv_channels_last_kernel");
    hipLaunchKernelGGL(cv_sign_sweep_kernel, dim3((unsigned)cdiv(P, CV_POS), (unsigned)cdiv(D, CV_PLANES), (unsigned)B), dim3(256), 0, st, x,
                       ws.xa_cl, ws.pose, depth_bins, ws.masks, samples, A, H, W, Hf, Wf, D, fov_scale);
    MCR_LAUNCH_CHECK("cv_sign_sweep_kernel");
    if (d_x) {
        hipLaunchKernelGGL(cv_dx_kernel, dim3((unsigned)cdiv(P, CV_POS), (unsigned)B), dim3(256), 0, st, d_out, d_out_batch_stride, ws.masks,
                           ws.maxbits, d_x, P, D);
        MCR_LAUNCH_CHECK("cv_dx_kernel");
    }
    if (d_x_alpha) {
        const dim3 sg((unsigned)cdiv(n_samples, 256));
        hipLaunchKernelGGL(cv_scatter_kernel<false>, sg, dim3(256), 0, st, samples, d_out, d_out_batch_stride, ws.counts, ws.counts, ws.entries,
                           n_samples, A, Hf, Wf, D);
        MCR_LAUNCH_CHECK("cv_scatter_kernel<count>");
        hipLaunchKernelGGL(cv_scan_kernel, dim3(1), dim3(CV_SCAN_THREADS), 0, st, ws.counts, ws.cursor, n_dest);
        MCR_LAUNCH_CHECK("cv_scan_kernel");
        hipLaunchKernelGGL(cv_scatter_kernel<true>, sg, dim3(256), 0, st, samples, d_out, d_out_batch_stride, ws.cursor, ws.counts, ws.entries,
                           n_samples, A, Hf, Wf, D);
        MCR_LAUNCH_CHECK("cv_scatter_kernel<fill>");
        hipLaunchKernelGGL(cv_dest_sum_kernel, dim3((unsigned)cdiv(n_dest, CV_DEST_PER_WG)), dim3(256), 0, st, ws.counts, ws.entries, ws.masks,
                           ws.maxbits, ws.xa_cl, n_dest, A, P, D);
        MCR_LAUNCH_CHECK("cv_dest_sum_kernel");
        hipLaunchKernelGGL(cv_from_channels_last_kernel, dim3((unsigned)cdiv(P, 64), (unsigned)(B * A)), dim3(256), 0, st, ws.xa_cl, d_x_alpha, P);
        MCR_LAUNCH_CHECK("cv_from_channels_last_kernel");
    }
    return 0;
}
