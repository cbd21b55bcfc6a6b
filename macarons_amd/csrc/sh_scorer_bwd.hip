// K9 backward — gradients of the SH coverage-gain scorer (sh_scorer.hip) for gfx950 (MI355X).
//
// The trainers differentiate through SconeVis.compute_coverage_gain / compute_visibilities
// (macarons/trainers/pretrain_scone_vis.py:168-224, train_macarons.py:1259 via macarons_utils.py:1678-1704).  With
//   z[b,c,n] = sum_k Y_k(dir(cams[b,c] - pts[b,n,:3])) h[b,n,k],   out = act(z),   s = act'(z) * weight[b,c,n]
// (weight = grad[b,c] / N for the gains, grad[b,c,n] for the per-pair visibilities; act' = sigma (1 - sigma), or 1 where z > 0 and 0
// elsewhere for relu -- torch's threshold_backward) the three gradients are
//   d_harm[b,n,:] =  sum_c s Y(dir)
//   d_cams[b,c,:] =  sum_n s grad_d z,      d_pts[b,n,:3] = -sum_c s grad_d z,     grad_d z = (g - (n.g) n) / |d|,  g = grad_n z.
//
// Layout of the work: one lane owns one point, as in the forward.  A unit is (cloud, wave-tile of 64 points, chunk of cameras); one
// wave runs one unit.  Per pair the lane adds s x^k {Re, Im}(w^m) into 64 accumulators G -- the gradient with respect to the
// monomial coefficients a of sh_mono.h (dz/da[shk(m+k, +-m)] = x^k {Re, Im} w^m, x = n_y, w = n_z + i n_x): no Y_k is ever evaluated.
// At the end of the unit G goes through the transpose of the coefficient transform (from_mono_grads) and out through the LDS strip.
// The transform is linear, so a point whose cameras are split over several chunks transforms each chunk's G and the chunks' rows are
// added in chunk order by a second pass.  The direction gradient comes from derivative Horner chains over the same a (sh_dot_dn).
//
// Deterministic: every partial sum has one writer and is added in a fixed order (no float atomics); the chunking is a function of
// (B, N, C) alone, so it does not depend on the device either.
#include "sh_mono.h"
#include <algorithm>

namespace mcr {

constexpr int SB_BLOCK = 256;                        // 4 waves, one unit each
constexpr long long SB_TARGET_WAVES = 3072;          // 256 CUs x 4 SIMDs x 3 waves (the d_harm kernel's occupancy)
constexpr long long SB_MIN_CAMS = 4;                 // cameras per chunk at least: the tile load and the transforms are per chunk
constexpr long long SB_CHUNK_BUDGET = 32ll << 20;    // bytes of per-chunk partials at most (d_harm and d_pts rows)

// z and g = grad_n z, z read as a polynomial in (n_x, n_y, n_z).  With P_m = U_m - i V_m (sh_mono.h) and x = n_y, w = n_z + i n_x:
//   z = U_0(x) + Re(w Q),  Q = sum_{m>=1} w^{m-1} P_m(x)
//   dz/dx = U_0'(x) + Re(w E),  E = sum_{m>=1} w^{m-1} P_m'(x)
//   F = w Q:  dz/dn_z = Re F',  dz/dn_x = -Im F',  F' = Q + w D,  D = dQ/dw
// Q, D and E are one complex Horner pass over the orders; U_m, V_m and their x-derivatives one real Horner pass each.
__device__ __forceinline__ float sh_dot_dn(float nx, float ct, float nz, const float (&a)[64], float& gx, float& gy, float& gz) {
    float z = a[shk(7, 0)], zd = 0.f;
#pragma unroll
    for (int l = 6; l >= 0; --l) {
        zd = fmaf(ct, zd, z);
        z = fmaf(ct, z, a[shk(l, 0)]);
    }
    // A = Q = ar - i bi, D = dr - i di, E = er - i ei;  P_7 is a constant: P_7' = 0
    float ar = a[shk(7, 7)], bi = a[shk(7, -7)], dr = 0.f, di = 0.f, er = 0.f, ei = 0.f;
#pragma unroll
    for (int m = 6; m >= 1; --m) {
        float U = a[shk(7, m)], V = a[shk(7, -m)], Ud = 0.f, Vd = 0.f;
#pragma unroll
        for (int l = 6; l >= m; --l) {
            Ud = fmaf(ct, Ud, U);
            Vd = fmaf(ct, Vd, V);
            U = fmaf(ct, U, a[shk(l, m)]);
            V = fmaf(ct, V, a[shk(l, -m)]);
        }
        const float ndr = fmaf(dr, nz, fmaf(di, nx, ar));          // D <- D w + A (the old A)
        const float ndi = fmaf(di, nz, fmaf(-dr, nx, bi));
        const float ner = fmaf(er, nz, fmaf(ei, nx, Ud));          // E <- E w + P_m'
        const float nei = fmaf(ei, nz, fmaf(-er, nx, Vd));
        const float nr = fmaf(ar, nz, fmaf(bi, nx, U));            // A <- A w + P_m
        const float nb = fmaf(bi, nz, fmaf(-ar, nx, V));
        dr = ndr; di = ndi; er = ner; ei = nei; ar = nr; bi = nb;
    }
    gy = fmaf(nz, er, fmaf(nx, ei, zd));
    gz = fmaf(nz, dr, fmaf(nx, di, ar));
    gx = fmaf(nz, di, fmaf(-nx, dr, bi));
    return fmaf(nz, ar, fmaf(nx, bi, z));
}

// G[shk(m+k, +-m)] += s x^k {Re, Im} w^m: 64 FMAs and the powers.
__device__ __forceinline__ void add_mono_grads(float s, float nx, float ct, float nz, float (&G)[64]) {
    float xs[8];
    xs[0] = s;
#pragma unroll
    for (int k = 1; k < 8; ++k) xs[k] = xs[k - 1] * ct;
#pragma unroll
    for (int k = 0; k < 8; ++k) G[shk(k, 0)] += xs[k];
    float wr = nz, wi = nx;
#pragma unroll
    for (int m = 1; m < 8; ++m) {
#pragma unroll
        for (int k = 0; k + m < 8; ++k) {
            G[shk(m + k, m)] = fmaf(xs[k], wr, G[shk(m + k, m)]);
            G[shk(m + k, -m)] = fmaf(xs[k], wi, G[shk(m + k, -m)]);
        }
        if (m < 7) {
            const float nwr = fmaf(wr, nz, -wi * nx), nwi = fmaf(wi, nz, wr * nx);
            wr = nwr; wi = nwi;
        }
    }
}

// NEED_H: d_harm rows -> out_h (d_harm itself, or the chunk's slice of the partials); NEED_DIR: the direction gradient, for d_pts
// (need_p: rows of p_stride floats -> out_p, channels >= 3 set to 0) and / or d_cams (need_c: per-(camera, wave-tile) wave sums ->
// part_c[b][c][xyz][wave-tile]).  Blank lanes (past N) carry the cloud's last point with weight 0: s = 0 exactly and their
// direction gradient is finite, so they add exactly 0 to the wave sums.  sigma' is sigma (1 - sigma): finite for every z.
template <bool SIGMOID, bool NEED_H, bool NEED_DIR>
__global__ __launch_bounds__(SB_BLOCK) void sh_bwd_kernel(const float* __restrict__ pts, int pts_stride, const float* __restrict__ harm,
                                                          const float* __restrict__ cams, const float* __restrict__ grad, int per_pair,
                                                          float inv_n, float* __restrict__ out_h, float* __restrict__ out_p, int p_stride,
                                                          float* __restrict__ part_c, int need_p, int need_c, int B, int N, int C,
                                                          int n_wtiles, int n_chunks, int chunk_len) {
    __shared__ ScStage s_stage[SB_BLOCK / MCR_WAVE];
    const int lane = threadIdx.x & (MCR_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / MCR_WAVE);
    const long long u = (long long)blockIdx.x * (SB_BLOCK / MCR_WAVE) + wave;
    if (u >= (long long)B * n_wtiles * n_chunks) return;
    const int chunk = __builtin_amdgcn_readfirstlane((int)(u % n_chunks));
    const long long bt = u / n_chunks;
    const int wt = __builtin_amdgcn_readfirstlane((int)(bt % n_wtiles));
    const int b = __builtin_amdgcn_readfirstlane((int)(bt / n_wtiles));
    const int c0 = chunk * chunk_len, c1 = min(C, c0 + chunk_len);
    const int n = wt * MCR_WAVE + lane;
    const bool valid = n < N;
    const int nc = valid ? n : N - 1;
    const size_t pn = (size_t)b * N + nc;

    float a[64];
    load_tile_rows(harm + (size_t)b * N * 64, wt * MCR_WAVE, N, lane, s_stage[wave], a);
    const float px = pts[pn * pts_stride + 0], py = pts[pn * pts_stride + 1], pz = pts[pn * pts_stride + 2];
    to_mono_coeffs<false>(a);

    float G[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) G[k] = 0.f;
    float dpx = 0.f, dpy = 0.f, dpz = 0.f;
    const float* cam_b = cams + (size_t)b * C * 3;
    const float* g_b = grad + (per_pair ? (size_t)b * C * N + nc : (size_t)b * C);
    const float lane_w = valid ? 1.f : 0.f;
    for (int c = c0; c < c1; ++c) {
        const float dx = cam_b[3 * c + 0] - px, dy = cam_b[3 * c + 1] - py, dz = cam_b[3 * c + 2] - pz;   // rays = X_cam - X_pts
        const float wgt = lane_w * (per_pair ? g_b[(size_t)c * N] : g_b[c] * inv_n);
        const float ir = __builtin_amdgcn_rsqf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        const float nx = dx * ir, ct = dy * ir, nz = dz * ir;
        float gx = 0.f, gy = 0.f, gz = 0.f, z;
        if (NEED_DIR) z = sh_dot_dn(nx, ct, nz, a, gx, gy, gz);
        else z = sh_dot(dx, dy, dz, a);                              // the same normalisation: shared with the lines above
        float s;
        if (SIGMOID) {
            const float sg = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
            s = sg * (1.f - sg) * wgt;
        } else {
            s = z > 0.f ? wgt : 0.f;
        }
        if (NEED_H) add_mono_grads(s, nx, ct, nz, G);
        if (NEED_DIR) {
            const float ng = fmaf(nx, gx, fmaf(ct, gy, nz * gz));
            const float f = s * ir;
            float t[3] = {f * fmaf(-ng, nx, gx), f * fmaf(-ng, ct, gy), f * fmaf(-ng, nz, gz)};
            dpx -= t[0]; dpy -= t[1]; dpz -= t[2];
            if (need_c) {
                wave_sum_to_last_multi<3>(t);
                if (lane == MCR_WAVE - 1) {
                    float* pc = part_c + ((size_t)b * C + c) * 3 * n_wtiles + wt;
                    pc[0] = t[0]; pc[n_wtiles] = t[1]; pc[2 * (size_t)n_wtiles] = t[2];
                }
            }
        }
    }
    if (NEED_H) {
        from_mono_grads(G);
        store_tile_rows(out_h + ((size_t)chunk * B + b) * N * 64, wt * MCR_WAVE, N, lane, s_stage[wave], G);
    }
    if (NEED_DIR && need_p && valid) {
        float* o = out_p + (((size_t)chunk * B + b) * N + n) * p_stride;
        o[0] = dpx; o[1] = dpy; o[2] = dpz;
        for (int j = 3; j < p_stride; ++j) o[j] = 0.f;
    }
}

// out[i] = sum over the chunks of part[chunk][i], in chunk order (float4 elements).
__global__ __launch_bounds__(256) void sh_bwd_sum_chunks_kernel(const float4* __restrict__ part, float4* __restrict__ out, long long n4,
                                                                int n_chunks) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 acc = part[i];
        for (int k = 1; k < n_chunks; ++k) {
            const float4 v = part[(size_t)k * n4 + i];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        out[i] = acc;
    }
}

// d_pts[b,n,:] = sum over the chunks of part[chunk][b,n,0:3] in chunk order; channels >= 3 get 0.
__global__ __launch_bounds__(256) void sh_bwd_sum_pts_kernel(const float* __restrict__ part, float* __restrict__ out, long long BN,
                                                             int n_chunks, int pts_dim) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < BN; i += (long long)gridDim.x * 256) {
        float acc[3] = {part[3 * i], part[3 * i + 1], part[3 * i + 2]};
        for (int k = 1; k < n_chunks; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j] += part[((size_t)k * BN + i) * 3 + j];
        for (int j = 0; j < pts_dim; ++j) out[i * pts_dim + j] = j < 3 ? acc[j] : 0.f;
    }
}

// d_cams[b,c,j] = sum_wt part_c[b][c][j][wt]; one block per (b, c), fixed tree order in fp64 (as sh_reduce_kernel).
__global__ __launch_bounds__(256) void sh_bwd_cams_reduce_kernel(const float* __restrict__ part, float* __restrict__ d_cams, int n_wtiles,
                                                                 int C) {
    __shared__ double s_w[3][4];
    const int c = blockIdx.x, b = blockIdx.y;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* p = part + (((size_t)b * C + c) * 3 + j) * n_wtiles;
        double acc = 0.0;
        for (int t = threadIdx.x; t < n_wtiles; t += 256) acc += (double)p[t];
        acc = wave_sum_all(acc);
        if ((threadIdx.x & 63) == 0) s_w[j][threadIdx.x >> 6] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int j = threadIdx.x;
        d_cams[((size_t)b * C + c) * 3 + j] = (float)four_wave_sum(s_w[j]);
    }
}

struct BwdPlan {
    int n_wtiles, n_chunks, chunk_len;
    size_t part_h, part_p, part_c;                   // bytes of each workspace region, in this order
};

static BwdPlan bwd_plan(int64_t B, int64_t N, int64_t C) {
    BwdPlan p;
    p.n_wtiles = (int)cdiv(N, MCR_WAVE);
    const long long tiles = (long long)B * p.n_wtiles, row_bytes = (long long)B * N * (64 + 3) * (long long)sizeof(float);
    long long k = std::min<long long>(cdiv(SB_TARGET_WAVES, tiles), cdiv(C, SB_MIN_CAMS));
    k = std::max<long long>(1, std::min<long long>(k, SB_CHUNK_BUDGET / row_bytes));
    p.chunk_len = (int)cdiv(C, k);
    p.n_chunks = (int)cdiv(C, p.chunk_len);
    p.part_h = p.n_chunks > 1 ? (size_t)p.n_chunks * B * N * 64 * sizeof(float) : 0;
    p.part_p = p.n_chunks > 1 ? (size_t)p.n_chunks * B * N * 3 * sizeof(float) : 0;
    p.part_c = (size_t)B * C * 3 * p.n_wtiles * sizeof(float);
    return p;
}

template <bool SIGMOID, bool NEED_H, bool NEED_DIR>
static void launch_bwd(dim3 grid, hipStream_t s, const float* pts, int pts_dim, const float* harm, const float* cams, const float* grad,
                       int per_pair, float inv_n, float* out_h, float* out_p, int p_stride, float* part_c, int need_p, int need_c, int B,
                       int N, int C, const BwdPlan& p) {
    hipLaunchKernelGGL((sh_bwd_kernel<SIGMOID, NEED_H, NEED_DIR>), grid, dim3(SB_BLOCK), 0, s, pts, pts_dim, harm, cams, grad, per_pair,
                       inv_n, out_h, out_p, p_stride, part_c, need_p, need_c, B, N, C, p.n_wtiles, p.n_chunks, p.chunk_len);
}

}  // namespace mcr

using namespace mcr;

extern "C" {

size_t mcr_sh_scorer_backward_workspace_bytes(int64_t B, int64_t N, int64_t C) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    const BwdPlan p = bwd_plan(B, N, C);
    return p.part_h + p.part_p + p.part_c;
}

int mcr_sh_scorer_backward(const float* pts, int pts_dim, const float* harmonics, const float* cams, const float* grad, int grad_per_pair,
                           int use_sigmoid, float* d_harm, float* d_pts, float* d_cams, int64_t B, int64_t N, int64_t C, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* who = "mcr_sh_scorer_backward";
    MCR_REQUIRE(pts && harmonics && cams && grad, "%s: null pointer", who);
    MCR_REQUIRE(pts_dim >= 3, "%s: pts_dim must be >= 3 (got %d)", who, pts_dim);
    MCR_REQUIRE(B > 0 && N > 0 && C > 0, "%s: empty problem B=%ld N=%ld C=%ld", who, (long)B, (long)N, (long)C);
    // N <= 2^23: load_tile_rows addresses a coefficient row as a 32-bit byte offset (row * 256) from the cloud's base
    MCR_REQUIRE(C <= 65535 && N <= (1ll << 23) && B <= 65535, "%s: problem too large (N <= 2^23, C <= 65535)", who);
    const BwdPlan p = bwd_plan(B, N, C);
    MCR_REQUIRE(workspace || p.part_h + p.part_p + p.part_c == 0, "%s: null workspace", who);
    MCR_REQUIRE(workspace_bytes >= p.part_h + p.part_p + p.part_c, "%s: workspace too small", who);
    const bool need_h = d_harm != nullptr, need_p = d_pts != nullptr, need_c = d_cams != nullptr, need_dir = need_p || need_c;
    if (!need_h && !need_dir) return 0;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* part_h = (float*)ws;
    float* part_p = (float*)(ws + p.part_h);
    float* part_c = (float*)(ws + p.part_h + p.part_p);
    const bool chunked = p.n_chunks > 1;
    float* out_h = chunked ? part_h : d_harm;
    float* out_p = chunked ? part_p : d_pts;
    const int p_stride = chunked ? 3 : pts_dim;
    const long long units = (long long)B * p.n_wtiles * p.n_chunks;
    const dim3 grid((unsigned)cdiv(units, SB_BLOCK / MCR_WAVE));
    const float inv_n = 1.0f / (float)N;
    const int iB = (int)B, iN = (int)N, iC = (int)C, pp = grad_per_pair ? 1 : 0, np = need_p ? 1 : 0, nc = need_c ? 1 : 0;
#define MCR_BWD_ARGS grid, s, pts, pts_dim, harmonics, cams, grad, pp, inv_n, out_h, out_p, p_stride, part_c, np, nc, iB, iN, iC, p
    if (use_sigmoid) {
        if (need_h && need_dir) launch_bwd<true, true, true>(MCR_BWD_ARGS);
        else if (need_h) launch_bwd<true, true, false>(MCR_BWD_ARGS);
        else launch_bwd<true, false, true>(MCR_BWD_ARGS);
    } else {
        if (need_h && need_dir) launch_bwd<false, true, true>(MCR_BWD_ARGS);
        else if (need_h) launch_bwd<false, true, false>(MCR_BWD_ARGS);
        else launch_bwd<false, false, true>(MCR_BWD_ARGS);
    }
#undef MCR_BWD_ARGS
    MCR_LAUNCH_CHECK("sh_bwd_kernel");
    if (chunked && need_h) {
        const long long n4 = B * N * 16;
        hipLaunchKernelGGL(sh_bwd_sum_chunks_kernel, dim3((unsigned)std::min<long long>(cdiv(n4, 256), 4096)), dim3(256), 0, s,
                           (const float4*)part_h, (float4*)d_harm, n4, p.n_chunks);
        MCR_LAUNCH_CHECK("sh_bwd_sum_chunks_kernel");
    }
    if (chunked && need_p) {
        hipLaunchKernelGGL(sh_bwd_sum_pts_kernel, dim3((unsigned)std::min<long long>(cdiv(B * N, 256), 4096)), dim3(256), 0, s, part_p,
                           d_pts, B * N, p.n_chunks, pts_dim);
        MCR_LAUNCH_CHECK("sh_bwd_sum_pts_kernel");
    }
    if (need_c) {
        hipLaunchKernelGGL(sh_bwd_cams_reduce_kernel, dim3((unsigned)C, (unsigned)B), dim3(256), 0, s, part_c, d_cams, p.n_wtiles, iC);
        MCR_LAUNCH_CHECK("sh_bwd_cams_reduce_kernel");
    }
    return 0;
}

}  // extern "C"
