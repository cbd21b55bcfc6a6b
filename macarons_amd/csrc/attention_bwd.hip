// Attention backward for gfx950 (MI355X), a building block of the networks' backward passes behind its own C entry points
// (include/macarons_hip.h: mcr_attention_backward, mcr_attention_backward_pct):
//   attention   flash-style: a stash-writing forward (O and LSE per (row, head)), then a query-major pass for dQ (and
//               delta = rowsum(dO * O)) and a key-major pass for dK, dV.  P = exp(S - LSE) is recomputed tile by tile; nothing
//               N x N is ever stored.  One lane owns one query (or key) row of one head; the 4 waves of a block share the row
//               block and split the other side's rows, their partial results meet in LDS in a fixed order.
// (Numerics and determinism: as stated in scone_vis_bwd.hip, for every entry of the backward sources.)
// The attention kernels are compiled for the per-head widths (16, 64) and (8, 32).  Sequences of 16 tokens have a fused attention
// backward of their own (a16_bwd_kernel: one wave per sequence, nothing but d_qkv written).
#include "bwd_kernels.h"

namespace mcr {
namespace {
typedef float f2 __attribute__((ext_vector_type(2)));

// The attention kernels are compiled for two pairs of per-head widths <DQ (q, k), DV (v)>: (16, 64) SconeVis, (8, 32) PCTransformer
constexpr int AB_TILE = 32;                            // keys (queries) staged per wave and step
template <int DQ> constexpr float ab_scale() { return DQ == 16 ? 0.25f : 0.35355339059327379f; }   // 1 / sqrt(DQ), DQ = 16 or 8

// ---- attention -----------------------------------------------------------------------------------------------------------------------
// Packed rows qkv[m*ldq + ...] = [q (H*DQ) | k (H*DQ) | v (H*DV)], head h owning q / k channels h*DQ.. and v channels h*DV..;
// S sequences of L rows; keys of sequence s: its first kmax = min(L, max(1, lens[s])) rows.  Grid (row blocks of 64, H, S), 4 waves.
__device__ __forceinline__ int ab_kmax(const int* lens, long long s, int L) { return lens ? min(L, max(1, lens[s])) : L; }

template <int N2>
__device__ __forceinline__ void ab_load(const float* p, f2 (&d)[N2], float scale) {
#pragma unroll
    for (int c = 0; c < N2 / 2; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * c);
        d[2 * c] = f2{v.x * scale, v.y * scale};
        d[2 * c + 1] = f2{v.z * scale, v.w * scale};
    }
}

template <int N2>
__device__ __forceinline__ float ab_dotq(const f2 (&a)[N2], const float* b) {
    f2 acc{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < N2 / 2; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(b + 4 * c);
        acc = __builtin_elementwise_fma(a[2 * c], f2{v.x, v.y}, acc);
        acc = __builtin_elementwise_fma(a[2 * c + 1], f2{v.z, v.w}, acc);
    }
    return acc.x + acc.y;
}

template <int N2>
__device__ __forceinline__ float ab_dotv(const f2 (&a)[N2], const float* b) {
    f2 acc0{0.f, 0.f}, acc1{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < N2 / 2; c += 2) {
        const float4 v = *reinterpret_cast<const float4*>(b + 4 * c);
        const float4 u = *reinterpret_cast<const float4*>(b + 4 * c + 4);
        acc0 = __builtin_elementwise_fma(a[2 * c], f2{v.x, v.y}, acc0);
        acc1 = __builtin_elementwise_fma(a[2 * c + 1], f2{v.z, v.w}, acc1);
        acc0 = __builtin_elementwise_fma(a[2 * c + 2], f2{u.x, u.y}, acc0);
        acc1 = __builtin_elementwise_fma(a[2 * c + 3], f2{u.z, u.w}, acc1);
    }
    const f2 t = acc0 + acc1;
    return t.x + t.y;
}

template <int N2>
__device__ __forceinline__ void ab_axpy(f2 (&y)[N2], float a, const float* x) {
    const f2 aa{a, a};
#pragma unroll
    for (int c = 0; c < N2 / 2; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(x + 4 * c);
        y[2 * c] = __builtin_elementwise_fma(aa, f2{v.x, v.y}, y[2 * c]);
        y[2 * c + 1] = __builtin_elementwise_fma(aa, f2{v.z, v.w}, y[2 * c + 1]);
    }
}

// stage rows [r0, r0 + AB_TILE) (rows >= rmax as zeros) of n4 float4 per row from src (row stride ld floats) into dst [AB_TILE][4*n4]
template <int N4>
__device__ __forceinline__ void ab_stage(float* dst, const float* src, long long ld, int r0, int rmax, int lane, float scale) {
#pragma unroll
    for (int e = lane; e < AB_TILE * N4; e += 64) {
        const int rr = e / N4, c4 = e - rr * N4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + rr < rmax) {
            v = *reinterpret_cast<const float4*>(src + (long long)(r0 + rr) * ld + 4 * c4);
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        }
        *reinterpret_cast<float4*>(dst + rr * 4 * N4 + 4 * c4) = v;
    }
}

// Small problems (fewer than 512 blocks of 64 rows: one or two 2048-token clouds) split the other side's rows over 2 or 4 blocks, so that
// every SIMD gets a wave; the parts are merged in part order by ab_fwd_merge_kernel / ab_sum_parts_kernel (a function of the shape
// alone: determinism).  Part sp of nsplit takes row tiles [t_lo, t_hi) of the n rows' ceil(n / AB_TILE) tiles.
inline int ab_nsplit(int64_t S, int L, int H) {
    const int64_t blocks = S * H * cdiv(L, 64);
    return blocks >= 512 ? 1 : blocks >= 256 ? 2 : 4;
}
__device__ __forceinline__ void ab_part_tiles(int n, int nsplit, int sp, int& t_lo, int& t_hi) {
    const int tiles = (n + AB_TILE - 1) / AB_TILE, per = (tiles + nsplit - 1) / nsplit;
    t_lo = min(tiles, sp * per);
    t_hi = min(tiles, t_lo + per);
}

// O = (sum_p e^{m_p - m} o_p) / l, LSE = m + log l, l = sum_p e^{m_p - m} l_p over the key parts, in part order; one thread per (row, head)
template <int DV>
__global__ __launch_bounds__(256) void ab_fwd_merge_kernel(const float* __restrict__ part, int nsplit, long long TH, int H, float* __restrict__ O,
                                                           long long ldo, float* __restrict__ lse) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= TH) return;
    const long long row = e / H;
    const int h = (int)(e - row * H);
    float m = -INFINITY, l = 0.f, o[DV];
#pragma unroll
    for (int c = 0; c < DV; ++c) o[c] = 0.f;
    for (int p = 0; p < nsplit; ++p) {
        const float* pp = part + (p * TH + e) * (DV + 2);
        const float m2 = pp[0];
        if (m2 == -INFINITY) continue;
        const float mn = fmaxf(m, m2), a1 = __expf(m - mn), a2 = __expf(m2 - mn);
        l = l * a1 + pp[1] * a2;
#pragma unroll
        for (int c = 0; c < DV; ++c) o[c] = o[c] * a1 + pp[2 + c] * a2;
        m = mn;
    }
    const float inv = 1.0f / l;
    float* op = O + row * ldo + h * DV;
#pragma unroll
    for (int c = 0; c < DV; ++c) op[c] = o[c] * inv;
    lse[e] = m + logf(l);
}

// out[r*ldo + c] = scale * sum_p part[(p*rows + r)*C + c], parts in order
__global__ __launch_bounds__(256) void ab_sum_parts_kernel(const float* __restrict__ part, int nsplit, long long rows, int C, float scale,
                                                           float* __restrict__ out, long long ldo) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * C) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    float acc = 0.f;
    for (int p = 0; p < nsplit; ++p) acc += part[p * rows * C + e];
    out[r * ldo + c] = acc * scale;
}

template <int DQ, int DV> constexpr int AB_KV_TILE = AB_TILE * (DQ + DV);            // floats of one wave's K | V tile
template <int DQ, int DV> constexpr int AB_FWD_LDS = 3 * 64 * (DV + 2);                   // the combine buffer (> 4 staging tiles)
static_assert(AB_FWD_LDS<16, 64> >= 4 * AB_KV_TILE<16, 64> && AB_FWD_LDS<8, 32> >= 4 * AB_KV_TILE<8, 32>, "LDS plan");

// O = softmax(q k^T / sqrt(DQ)) v and LSE = m + log(l) per (row, head).  Each wave runs the key tiles w, w + 4, ... with an online soft-max.
template <int DQ, int DV>
__global__ __launch_bounds__(256) void ab_fwd_kernel(const float* __restrict__ qkv, long long ldq, float* __restrict__ O, long long ldo,
                                                     float* __restrict__ lse, int L, int H, const int* __restrict__ lens,
                                                     float* __restrict__ part, int nsplit) {
    __shared__ float4 smem4[AB_FWD_LDS<DQ, DV> / 4];
    float* smem = reinterpret_cast<float*>(smem4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = blockIdx.y;
    const long long s = blockIdx.z / nsplit;
    const int sp = blockIdx.z - (int)s * nsplit;
    const int qi = blockIdx.x * 64 + lane;
    const int kmax = ab_kmax(lens, s, L);
    const int QK = H * DQ;
    const float* base = qkv + s * L * ldq;
    f2 q[DQ / 2];
    if (qi < L) ab_load(base + (long long)qi * ldq + h * DQ, q, ab_scale<DQ>());
    else
#pragma unroll
        for (int c = 0; c < DQ / 2; ++c) q[c] = f2{0.f, 0.f};
    f2 o[DV / 2];
#pragma unroll
    for (int c = 0; c < DV / 2; ++c) o[c] = f2{0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    float* kt = smem + w * AB_KV_TILE<DQ, DV>;
    float* vt = kt + AB_TILE * DQ;
    int t_lo, n_tiles;
    ab_part_tiles(kmax, nsplit, sp, t_lo, n_tiles);
    for (int t0 = t_lo; t0 < n_tiles; t0 += 4) {
        const int t = t0 + w;
        if (t < n_tiles) {
            ab_stage<DQ / 4>(kt, base + QK + h * DQ, ldq, t * AB_TILE, kmax, lane, 1.f);
            ab_stage<DV / 4>(vt, base + 2 * QK + h * DV, ldq, t * AB_TILE, kmax, lane, 1.f);
        }
        __syncthreads();
        if (t < n_tiles) {
            const int nk = min(AB_TILE, kmax - t * AB_TILE);
            float sc[AB_TILE];
            float mt = m;
#pragma unroll
            for (int j = 0; j < AB_TILE; ++j) {
                sc[j] = j < nk ? ab_dotq(q, kt + j * DQ) : -INFINITY;
                mt = fmaxf(mt, sc[j]);
            }
            const float alpha = __expf(m - mt);
            l *= alpha;
            const f2 aa{alpha, alpha};
#pragma unroll
            for (int c = 0; c < DV / 2; ++c) o[c] *= aa;
#pragma unroll
            for (int j = 0; j < AB_TILE; ++j) {
                const float p = __expf(sc[j] - mt);
                l += p;
                ab_axpy(o, p, vt + j * DV);
            }
            m = mt;
        }
        __syncthreads();
    }
    constexpr int F = DV + 2;
    if (w > 0) {
        float* cb = smem + (w - 1) * F * 64;
        cb[lane] = m;
        cb[64 + lane] = l;
#pragma unroll
        for (int c = 0; c < DV / 2; ++c) { cb[(2 + 2 * c) * 64 + lane] = o[c].x; cb[(3 + 2 * c) * 64 + lane] = o[c].y; }
    }
    __syncthreads();
    if (w == 0 && qi < L) {
        for (int k = 0; k < 3; ++k) {
            const float* cb = smem + k * F * 64;
            const float m2 = cb[lane];
            if (m2 == -INFINITY) continue;
            const float l2 = cb[64 + lane];
            const float mn = fmaxf(m, m2), a1 = __expf(m - mn), a2 = __expf(m2 - mn);
            l = l * a1 + l2 * a2;
#pragma unroll
            for (int c = 0; c < DV / 2; ++c) o[c] = o[c] * f2{a1, a1} + f2{cb[(2 + 2 * c) * 64 + lane], cb[(3 + 2 * c) * 64 + lane]} * f2{a2, a2};
            m = mn;
        }
        if (nsplit > 1) {                                              // this key part's (max, sum, unnormalised O): ab_fwd_merge_kernel
            const long long T = (long long)(gridDim.z / nsplit) * L;
            float* pp = part + ((sp * T + s * L + qi) * H + h) * (DV + 2);
            pp[0] = m;
            pp[1] = l;
#pragma unroll
            for (int c = 0; c < DV / 2; ++c) { pp[2 + 2 * c] = o[c].x; pp[3 + 2 * c] = o[c].y; }
            return;
        }
        const float inv = 1.0f / l;
        float* op = O + (s * L + qi) * ldo + h * DV;
#pragma unroll
        for (int c = 0; c < DV / 4; ++c)
            *reinterpret_cast<float4*>(op + 4 * c) = make_float4(o[2 * c].x * inv, o[2 * c].y * inv, o[2 * c + 1].x * inv, o[2 * c + 1].y * inv);
        lse[(s * L + qi) * H + h] = m + logf(l);
    }
}

// dQ pass (query-major): delta = rowsum(dO * O); for every key: p = exp(s - LSE), dp = dO . v, ds = p (dp - delta), dq += ds k / sqrt(DQ).
template <int DQ, int DV>
__global__ __launch_bounds__(256) void ab_dq_kernel(const float* __restrict__ qkv, long long ldq, const float* __restrict__ O, long long ldo,
                                                    const float* __restrict__ dO, long long lddo, const float* __restrict__ lse,
                                                    float* __restrict__ delta, float* __restrict__ dqkv, long long lddq, int L, int H,
                                                    const int* __restrict__ lens, float* __restrict__ part, int nsplit) {
    __shared__ float4 smem4[4 * AB_KV_TILE<DQ, DV> / 4];
    float* smem = reinterpret_cast<float*>(smem4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = blockIdx.y;
    const long long s = blockIdx.z / nsplit;
    const int sp = blockIdx.z - (int)s * nsplit;
    const int qi = blockIdx.x * 64 + lane;
    const int kmax = ab_kmax(lens, s, L);
    const int QK = H * DQ;
    const float* base = qkv + s * L * ldq;
    f2 q[DQ / 2], g[DV / 2];
    float lq = 0.f, dl = 0.f;
    if (qi < L) {
        const long long row = s * L + qi;
        ab_load(base + (long long)qi * ldq + h * DQ, q, ab_scale<DQ>());
        const float* gp = dO + row * lddo + h * DV;
        const float* op = O + row * ldo + h * DV;
        f2 d2{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DV / 4; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(gp + 4 * c);
            const float4 b = *reinterpret_cast<const float4*>(op + 4 * c);
            g[2 * c] = f2{a.x, a.y};
            g[2 * c + 1] = f2{a.z, a.w};
            d2 = __builtin_elementwise_fma(g[2 * c], f2{b.x, b.y}, d2);
            d2 = __builtin_elementwise_fma(g[2 * c + 1], f2{b.z, b.w}, d2);
        }
        dl = d2.x + d2.y;
        lq = lse[row * H + h];
    } else {
#pragma unroll
        for (int c = 0; c < DQ / 2; ++c) q[c] = f2{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DV / 2; ++c) g[c] = f2{0.f, 0.f};
    }
    f2 dq[DQ / 2];
#pragma unroll
    for (int c = 0; c < DQ / 2; ++c) dq[c] = f2{0.f, 0.f};
    float* kt = smem + w * AB_KV_TILE<DQ, DV>;
    float* vt = kt + AB_TILE * DQ;
    int t_lo, n_tiles;
    ab_part_tiles(kmax, nsplit, sp, t_lo, n_tiles);
    for (int t0 = t_lo; t0 < n_tiles; t0 += 4) {
        const int t = t0 + w;
        if (t < n_tiles) {
            ab_stage<DQ / 4>(kt, base + QK + h * DQ, ldq, t * AB_TILE, kmax, lane, 1.f);
            ab_stage<DV / 4>(vt, base + 2 * QK + h * DV, ldq, t * AB_TILE, kmax, lane, 1.f);
        }
        __syncthreads();
        if (t < n_tiles) {
            const int nk = min(AB_TILE, kmax - t * AB_TILE);
            for (int j = 0; j < nk; ++j) {
                const float p = __expf(ab_dotq(q, kt + j * DQ) - lq);
                const float ds = p * (ab_dotv(g, vt + j * DV) - dl);
                ab_axpy(dq, ds, kt + j * DQ);
            }
        }
        __syncthreads();
    }
    if (w > 0) {
        float* cb = smem + (w - 1) * DQ * 64;
#pragma unroll
        for (int c = 0; c < DQ / 2; ++c) { cb[(2 * c) * 64 + lane] = dq[c].x; cb[(2 * c + 1) * 64 + lane] = dq[c].y; }
    }
    __syncthreads();
    if (w == 0 && qi < L) {
        for (int k = 0; k < 3; ++k) {
            const float* cb = smem + k * DQ * 64;
#pragma unroll
            for (int c = 0; c < DQ / 2; ++c) dq[c] += f2{cb[(2 * c) * 64 + lane], cb[(2 * c + 1) * 64 + lane]};
        }
        const long long row = s * L + qi;
        const float sc = nsplit > 1 ? 1.f : ab_scale<DQ>();                  // (parts: scaled once summed, ab_sum_parts_kernel)
        float* dp = nsplit > 1 ? part + (sp * (long long)(gridDim.z / nsplit) * L + row) * QK + h * DQ : dqkv + row * lddq + h * DQ;
#pragma unroll
        for (int c = 0; c < DQ / 4; ++c)
            *reinterpret_cast<float4*>(dp + 4 * c) = make_float4(dq[2 * c].x * sc, dq[2 * c].y * sc, dq[2 * c + 1].x * sc, dq[2 * c + 1].y * sc);
        if (sp == 0) delta[row * H + h] = dl;
    }
}

template <int DQ, int DV> constexpr int AB_Q_TILE = AB_TILE * (DQ + DV + 2);          // floats of one wave's q | dO | LSE | delta tile
template <int DQ, int DV> constexpr int AB_KV_LDS = 3 * 64 * (DQ + DV);               // the combine buffer (> 4 staging tiles)
static_assert(AB_KV_LDS<16, 64> >= 4 * AB_Q_TILE<16, 64> && AB_KV_LDS<8, 32> >= 4 * AB_Q_TILE<8, 32>, "LDS plan");

// dK / dV pass (key-major): every query row of the sequence (padded ones included) against this lane's key.
template <int DQ, int DV>
__global__ __launch_bounds__(256) void ab_dkdv_kernel(const float* __restrict__ qkv, long long ldq, const float* __restrict__ dO, long long lddo,
                                                      const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dqkv,
                                                      long long lddq, int L, int H, const int* __restrict__ lens, float* __restrict__ part,
                                                      int nsplit) {
    __shared__ float4 smem4[AB_KV_LDS<DQ, DV> / 4];
    float* smem = reinterpret_cast<float*>(smem4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = blockIdx.y;
    const long long s = blockIdx.z / nsplit;
    const int sp = blockIdx.z - (int)s * nsplit;
    const int kj = blockIdx.x * 64 + lane;
    const int kmax = ab_kmax(lens, s, L);
    const int QK = H * DQ;
    const float* base = qkv + s * L * ldq;
    const bool live_block = blockIdx.x * 64 < kmax;               // (uniform) a block of keys beyond every cloud's keys: zeros
    f2 k[DQ / 2], v[DV / 2], dk[DQ / 2], dv[DV / 2];
#pragma unroll
    for (int c = 0; c < DQ / 2; ++c) dk[c] = f2{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DV / 2; ++c) dv[c] = f2{0.f, 0.f};
    if (kj < kmax) {
        ab_load(base + (long long)kj * ldq + QK + h * DQ, k, 1.f);
        const float* vp = base + (long long)kj * ldq + 2 * QK + h * DV;
#pragma unroll
        for (int c = 0; c < DV / 4; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(vp + 4 * c);
            v[2 * c] = f2{a.x, a.y};
            v[2 * c + 1] = f2{a.z, a.w};
        }
    } else {
#pragma unroll
        for (int c = 0; c < DQ / 2; ++c) k[c] = f2{0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DV / 2; ++c) v[c] = f2{0.f, 0.f};
    }
    float* qt = smem + w * AB_Q_TILE<DQ, DV>;
    float* gt = qt + AB_TILE * DQ;
    float* lt = gt + AB_TILE * DV;
    float* dt = lt + AB_TILE;
    int t_lo, n_tiles;
    ab_part_tiles(live_block ? L : 0, nsplit, sp, t_lo, n_tiles);
    for (int t0 = t_lo; t0 < n_tiles; t0 += 4) {
        const int t = t0 + w;
        if (t < n_tiles) {
            ab_stage<DQ / 4>(qt, base + h * DQ, ldq, t * AB_TILE, L, lane, ab_scale<DQ>());
            ab_stage<DV / 4>(gt, dO + s * L * lddo + h * DV, lddo, t * AB_TILE, L, lane, 1.f);
            if (lane < AB_TILE) {
                const int r = t * AB_TILE + lane;
                lt[lane] = r < L ? lse[(s * L + r) * H + h] : 0.f;
                dt[lane] = r < L ? delta[(s * L + r) * H + h] : 0.f;
            }
        }
        __syncthreads();
        if (t < n_tiles) {
            const int nq = min(AB_TILE, L - t * AB_TILE);
            for (int i = 0; i < nq; ++i) {
                const float p = __expf(ab_dotq(k, qt + i * DQ) - lt[i]);
                ab_axpy(dv, p, gt + i * DV);
                const float ds = p * (ab_dotv(v, gt + i * DV) - dt[i]);
                ab_axpy(dk, ds, qt + i * DQ);
            }
        }
        __syncthreads();
    }
    constexpr int F = DQ + DV;
    if (w > 0) {
        float* cb = smem + (w - 1) * F * 64;
#pragma unroll
        for (int c = 0; c < DQ / 2; ++c) { cb[(2 * c) * 64 + lane] = dk[c].x; cb[(2 * c + 1) * 64 + lane] = dk[c].y; }
#pragma unroll
        for (int c = 0; c < DV / 2; ++c) { cb[(DQ + 2 * c) * 64 + lane] = dv[c].x; cb[(DQ + 1 + 2 * c) * 64 + lane] = dv[c].y; }
    }
    __syncthreads();
    if (w == 0 && kj < L) {
        if (live_block)
            for (int kk = 0; kk < 3; ++kk) {
                const float* cb = smem + kk * F * 64;
#pragma unroll
                for (int c = 0; c < DQ / 2; ++c) dk[c] += f2{cb[(2 * c) * 64 + lane], cb[(2 * c + 1) * 64 + lane]};
#pragma unroll
                for (int c = 0; c < DV / 2; ++c) dv[c] += f2{cb[(DQ + 2 * c) * 64 + lane], cb[(DQ + 1 + 2 * c) * 64 + lane]};
            }
        if (kj >= kmax) {                                             // a key nobody attends to
#pragma unroll
            for (int c = 0; c < DQ / 2; ++c) dk[c] = f2{0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DV / 2; ++c) dv[c] = f2{0.f, 0.f};
        }
        // parts: rows [dk (QK) | dv (H * DV)] laid out as d_qkv from column QK on, summed by ab_sum_parts_kernel
        const int W2 = QK + H * DV;
        float* dkp = nsplit > 1 ? part + (sp * (long long)(gridDim.z / nsplit) * L + s * L + kj) * W2 : dqkv + (s * L + kj) * lddq + QK;
#pragma unroll
        for (int c = 0; c < DQ / 4; ++c)
            *reinterpret_cast<float4*>(dkp + h * DQ + 4 * c) = make_float4(dk[2 * c].x, dk[2 * c].y, dk[2 * c + 1].x, dk[2 * c + 1].y);
#pragma unroll
        for (int c = 0; c < DV / 4; ++c)
            *reinterpret_cast<float4*>(dkp + QK + h * DV + 4 * c) = make_float4(dv[2 * c].x, dv[2 * c].y, dv[2 * c + 1].x, dv[2 * c + 1].y);
    }
}

// part: ab_part_floats(S, L, H, DQ, DV) floats of scratch (none needed when the problem is not split)
template <int DQ, int DV>
void launch_attn_fwd_t(hipStream_t s, const float* qkv, int64_t ldq, float* O, int64_t ldo, float* lse, int64_t S, int L, int H, const int* lens,
                       float* part) {
    const int ns = ab_nsplit(S, L, H);
    hipLaunchKernelGGL((ab_fwd_kernel<DQ, DV>), dim3((unsigned)cdiv(L, 64), (unsigned)H, (unsigned)(S * ns)), dim3(256), 0, s, qkv, (long long)ldq,
                       O, (long long)ldo, lse, L, H, lens, part, ns);
    if (ns > 1) {
        const long long TH = S * L * H;
        hipLaunchKernelGGL(ab_fwd_merge_kernel<DV>, dim3((unsigned)cdiv(TH, 256)), dim3(256), 0, s, part, ns, TH, H, O, (long long)ldo, lse);
    }
}

template <int DQ, int DV>
void launch_attn_bwd_t(hipStream_t s, const float* qkv, int64_t ldq, const float* O, int64_t ldo, const float* lse, const float* dO,
                       int64_t lddo, float* delta, float* dqkv, int64_t lddq, int64_t S, int L, int H, const int* lens, float* part) {
    const int ns = ab_nsplit(S, L, H);
    const long long T = S * L;
    const int QK = H * DQ, W2 = QK + H * DV;
    const dim3 grid((unsigned)cdiv(L, 64), (unsigned)H, (unsigned)(S * ns));
    hipLaunchKernelGGL((ab_dq_kernel<DQ, DV>), grid, dim3(256), 0, s, qkv, (long long)ldq, O, (long long)ldo, dO, (long long)lddo, lse, delta, dqkv,
                       (long long)lddq, L, H, lens, part, ns);
    if (ns > 1)
        hipLaunchKernelGGL(ab_sum_parts_kernel, dim3((unsigned)cdiv(T * QK, 256)), dim3(256), 0, s, part, ns, T, QK, ab_scale<DQ>(), dqkv, (long long)lddq);
    hipLaunchKernelGGL((ab_dkdv_kernel<DQ, DV>), grid, dim3(256), 0, s, qkv, (long long)ldq, dO, (long long)lddo, lse, delta, dqkv, (long long)lddq, L,
                       H, lens, part, ns);
    if (ns > 1)
        hipLaunchKernelGGL(ab_sum_parts_kernel, dim3((unsigned)cdiv(T * W2, 256)), dim3(256), 0, s, part, ns, T, W2, 1.f, dqkv + QK,
                           (long long)lddq);
}

// ---- attention backward for 16-token sequences at per-head widths (8, 32): the PCTransformer's neighbourhoods ----------------------------
// One wave owns one sequence: lane = (head h = lane / 16, row = lane % 16), so a head's 16 rows are one DPP row and the 64 lanes are the
// sequence's 4 x 16 (head, row) pairs.  Nothing but d_qkv is written: no O, no LSE, no 16 x 16 matrix leaves the wave.
//   pass 1 (query-major): the lane keeps its own q (scaled) and dO in registers; the wave stages the sequence's K | V rows in its LDS
//           strip.  The lane rebuilds its 16 scores and their soft-max P, dP_j = dO . v_j, delta = sum_j P_j dP_j (= dO . O),
//           dS_j = P_j (dP_j - delta), and writes dq = sum_j dS_j k_j / sqrt(8).
//   pass 2 (key-major): the lane acts as key row j of its head.  P and dO, then dS and q, go through the strip (each lane writes its
//           row, reads column j of its head's rows 0..15 in that order): dv_j = sum_i P_ij dO_i, dk_j = sum_i dS_ij q_i / sqrt(8).
// The strip is private to the wave: wave-scope fences order its phases, there is no block barrier.  LDS reads of a pass are broadcasts
// within a head and hit four different banks across the heads ([row][head][channel] layouts; P / dS as [row i][head][j]: lane-linear).
// Registers: 242 VGPRs, no scratch, 2 waves per SIMD (the 48 KB strip block would allow 3; asking for 3 makes hipcc spill 288 bytes
// per lane, its schedule hoists the strip reads of the fully unrolled j loops).
constexpr int A16_L = 16, A16_H = 4, A16_DQ = 8, A16_DV = 32;
constexpr int A16_QK = A16_H * A16_DQ, A16_V = A16_H * A16_DV;     // 32 q (k) and 128 v channels of a packed row
constexpr int A16_STRIP = A16_L * 64 + A16_L * A16_V;              // floats per wave: P (or dS) [16][64] | dO [16][128] >= K [16][32] | V [16][128]
constexpr int A16_WAVES = 4;                                       // sequences per block
static_assert(A16_STRIP >= A16_L * (A16_QK + A16_V), "LDS plan");

__device__ __forceinline__ void a16_wave_sync() {                  // orders the wave's own LDS traffic (in-order per wave in hardware)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * A16_WAVES) void a16_bwd_kernel(const float* __restrict__ qkv, long long ldq, const float* __restrict__ dO,
                                                                 long long lddo, float* __restrict__ dqkv, long long lddq, long long S) {
    __shared__ float4 smem4[A16_WAVES * A16_STRIP / 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 4, r = lane & 15;
    const long long s = (long long)blockIdx.x * A16_WAVES + w;
    if (s >= S) return;                                            // (wave-uniform; no block barrier below)
    float* strip = reinterpret_cast<float*>(smem4) + w * A16_STRIP;
    float* kt = strip;                                             // pass 1: K [16][32]
    float* vt = strip + A16_L * A16_QK;                            //         V [16][128]
    const float* base = qkv + s * A16_L * ldq;
    // the sequence's K | V: 16 rows x 40 float4 (columns 32 .. 191 of the packed rows), 10 per lane
#pragma unroll
    for (int it = 0; it < A16_L * (A16_QK + A16_V) / 4 / 64; ++it) {
        const int e = lane + 64 * it;
        const int j = e / ((A16_QK + A16_V) / 4), c4 = e - j * ((A16_QK + A16_V) / 4);
        const float4 v = *reinterpret_cast<const float4*>(base + (long long)j * ldq + A16_QK + 4 * c4);
        float* dst = c4 < A16_QK / 4 ? kt + j * A16_QK + 4 * c4 : vt + j * A16_V + 4 * (c4 - A16_QK / 4);
        *reinterpret_cast<float4*>(dst) = v;
    }
    f2 q[A16_DQ / 2], g[A16_DV / 2];
    ab_load(base + (long long)r * ldq + h * A16_DQ, q, ab_scale<A16_DQ>());
    ab_load(dO + (s * A16_L + r) * lddo + h * A16_DV, g, 1.f);
    a16_wave_sync();
    float p[A16_L], ds[A16_L];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < A16_L; ++j) {
        p[j] = ab_dotq(q, kt + j * A16_QK + h * A16_DQ);
        m = fmaxf(m, p[j]);
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < A16_L; ++j) {
        p[j] = __expf(p[j] - m);
        l += p[j];
    }
    const float inv = 1.0f / l;
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < A16_L; ++j) {
        p[j] *= inv;
        ds[j] = ab_dotv(g, vt + j * A16_V + h * A16_DV);           // dP_j
        delta = fmaf(p[j], ds[j], delta);
    }
    f2 dq[A16_DQ / 2];
#pragma unroll
    for (int c = 0; c < A16_DQ / 2; ++c) dq[c] = f2{0.f, 0.f};
#pragma unroll
    for (int j = 0; j < A16_L; ++j) {
        ds[j] = p[j] * (ds[j] - delta);
        ab_axpy(dq, ds[j], kt + j * A16_QK + h * A16_DQ);
    }
    float* out = dqkv + (s * A16_L + r) * lddq;
    const float sc = ab_scale<A16_DQ>();
#pragma unroll
    for (int c = 0; c < A16_DQ / 4; ++c)
        *reinterpret_cast<float4*>(out + h * A16_DQ + 4 * c) =
            make_float4(dq[2 * c].x * sc, dq[2 * c].y * sc, dq[2 * c + 1].x * sc, dq[2 * c + 1].y * sc);
    // ---- pass 2a: dv_j = sum_i P_ij dO_i
    float* xt = strip;                                             // P, then dS: [i][h][j]
    float* gt = strip + A16_L * 64;                                // dO [i][h][32], then q [i][h][8]
    a16_wave_sync();                                               // every lane is done with K | V
#pragma unroll
    for (int c = 0; c < A16_L / 4; ++c)
        *reinterpret_cast<float4*>(xt + r * 64 + h * 16 + 4 * c) = make_float4(p[4 * c], p[4 * c + 1], p[4 * c + 2], p[4 * c + 3]);
#pragma unroll
    for (int c = 0; c < A16_DV / 4; ++c)
        *reinterpret_cast<float4*>(gt + r * A16_V + h * A16_DV + 4 * c) = make_float4(g[2 * c].x, g[2 * c].y, g[2 * c + 1].x, g[2 * c + 1].y);
    a16_wave_sync();
    f2 dv[A16_DV / 2];
#pragma unroll
    for (int c = 0; c < A16_DV / 2; ++c) dv[c] = f2{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < A16_L; ++i) ab_axpy(dv, xt[i * 64 + lane], gt + i * A16_V + h * A16_DV);
#pragma unroll
    for (int c = 0; c < A16_DV / 4; ++c)
        *reinterpret_cast<float4*>(out + 2 * A16_QK + h * A16_DV + 4 * c) = make_float4(dv[2 * c].x, dv[2 * c].y, dv[2 * c + 1].x, dv[2 * c + 1].y);
    // ---- pass 2b: dk_j = sum_i dS_ij q_i (q already carries 1 / sqrt(8))
    a16_wave_sync();                                               // every lane is done with P | dO
#pragma unroll
    for (int c = 0; c < A16_L / 4; ++c)
        *reinterpret_cast<float4*>(xt + r * 64 + h * 16 + 4 * c) = make_float4(ds[4 * c], ds[4 * c + 1], ds[4 * c + 2], ds[4 * c + 3]);
#pragma unroll
    for (int c = 0; c < A16_DQ / 4; ++c)
        *reinterpret_cast<float4*>(gt + r * A16_QK + h * A16_DQ + 4 * c) = make_float4(q[2 * c].x, q[2 * c].y, q[2 * c + 1].x, q[2 * c + 1].y);
    a16_wave_sync();
    f2 dk[A16_DQ / 2];
#pragma unroll
    for (int c = 0; c < A16_DQ / 2; ++c) dk[c] = f2{0.f, 0.f};
#pragma unroll
    for (int i = 0; i < A16_L; ++i) ab_axpy(dk, xt[i * 64 + lane], gt + i * A16_QK + h * A16_DQ);
#pragma unroll
    for (int c = 0; c < A16_DQ / 4; ++c)
        *reinterpret_cast<float4*>(out + A16_QK + h * A16_DQ + 4 * c) = make_float4(dk[2 * c].x, dk[2 * c].y, dk[2 * c + 1].x, dk[2 * c + 1].y);
}

// the workspace of the two entries (dq = 8 at L = 16: none, the 16-token kernel keeps everything in the wave)
struct AttnBwdScratch { float *O, *lse, *delta, *part; };
AttnBwdScratch carve_attention_backward(Arena& a, int64_t S, int64_t L, int n_heads, int v_dim, int dq) {
    AttnBwdScratch w{};
    if (dq == 8 && L == 16) return w;
    const int64_t T = S * L;
    w.O = a.f(T * v_dim);
    w.lse = a.f(T * n_heads);
    w.delta = a.f(T * n_heads);
    w.part = a.f(ab_part_floats(S, (int)L, n_heads, dq, 4 * dq));
    return w;
}
size_t ab_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim, int dq) {
    return measure(carve_attention_backward, S, L, n_heads, v_dim, dq) + VB_BLOCK_WS_SLACK;
}

// what the two entries share once their own widths and sizes are checked: the packed operands (rows covered, float4 accesses possible),
// the workspace, the launches at per-head widths (dq, 4 dq)
int ab_backward(const char* who, const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes, void* stream, int dq) {
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldq % 4 == 0 && ld_dout >= v_dim && ld_dout % 4 == 0 && ld_dqkv >= 2 * qk_dim + v_dim &&
                    ld_dqkv % 4 == 0,
                "%s: leading dimensions must cover the rows and be multiples of 4", who);
    MCR_REQUIRE(((uintptr_t)qkv | (uintptr_t)d_out | (uintptr_t)d_qkv) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (dq == 8 && L == 16) {
        launch_attn16_bwd(s, qkv, ldq, d_out, ld_dout, d_qkv, ld_dqkv, S);
        MCR_LAUNCH_CHECK(who);
        return 0;
    }
    if (check_bwd_workspace(who, workspace, workspace_bytes, ab_workspace_bytes(S, L, n_heads, v_dim, dq))) return 1;
    Arena a{(char*)workspace, workspace_bytes};
    const AttnBwdScratch ws = carve_attention_backward(a, S, L, n_heads, v_dim, dq);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    launch_attn_fwd(s, qkv, ldq, ws.O, v_dim, ws.lse, S, (int)L, n_heads, lens, ws.part, dq);
    launch_attn_bwd(s, qkv, ldq, ws.O, v_dim, ws.lse, d_out, ld_dout, ws.delta, d_qkv, ld_dqkv, S, (int)L, n_heads, lens, ws.part, dq);
    MCR_LAUNCH_CHECK(who);
    return 0;
}
}  // namespace

// ---- the launchers and the size function of bwd_kernels.h --------------------------------------------------------------------------------
size_t ab_part_floats(int64_t S, int L, int H, int dq, int dv) {
    const int ns = ab_nsplit(S, L, H);
    return ns > 1 ? (size_t)ns * S * L * H * (dq + dv) : 0;   // (>= the forward's H * (dv + 2) and the dq parts' H * dq per row)
}
void launch_attn_fwd(hipStream_t s, const float* qkv, int64_t ldq, float* O, int64_t ldo, float* lse, int64_t S, int L, int H, const int* lens,
                     float* part, int dq) {
    if (dq == 16) launch_attn_fwd_t<16, 64>(s, qkv, ldq, O, ldo, lse, S, L, H, lens, part);
    else launch_attn_fwd_t<8, 32>(s, qkv, ldq, O, ldo, lse, S, L, H, lens, part);
}
void launch_attn_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* O, int64_t ldo, const float* lse, const float* dO,
                     int64_t lddo, float* delta, float* dqkv, int64_t lddq, int64_t S, int L, int H, const int* lens, float* part, int dq) {
    if (dq == 16) launch_attn_bwd_t<16, 64>(s, qkv, ldq, O, ldo, lse, dO, lddo, delta, dqkv, lddq, S, L, H, lens, part);
    else launch_attn_bwd_t<8, 32>(s, qkv, ldq, O, ldo, lse, dO, lddo, delta, dqkv, lddq, S, L, H, lens, part);
}
void launch_attn16_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* dO, int64_t lddo, float* dqkv, int64_t lddq, int64_t S) {
    hipLaunchKernelGGL(a16_bwd_kernel, dim3((unsigned)cdiv(S, A16_WAVES)), dim3(64 * A16_WAVES), 0, s, qkv, (long long)ldq, dO, (long long)lddo,
                       dqkv, (long long)lddq, (long long)S);
}
}  // namespace mcr
using namespace mcr;
extern "C" {
size_t mcr_attention_backward_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim) { return ab_workspace_bytes(S, L, n_heads, v_dim, 16); }

int mcr_attention_backward(const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                           int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const char* who = "mcr_attention_backward";
    MCR_REQUIRE(qkv && d_out && d_qkv, "%s: null pointer", who);
    MCR_REQUIRE(n_heads > 0 && qk_dim == 16 * n_heads && v_dim == 64 * n_heads,
                "%s: per-head widths must be 16 (q, k) and 64 (v), got qk_dim %d, v_dim %d for %d heads", who, qk_dim, v_dim, n_heads);
    MCR_REQUIRE(S > 0 && L > 0 && S <= 65535 && L <= (1 << 30), "%s: bad problem size S=%ld L=%ld", who, (long)S, (long)L);
    return ab_backward(who, qkv, ldq, d_out, ld_dout, d_qkv, ld_dqkv, S, L, n_heads, qk_dim, v_dim, lens, workspace, workspace_bytes, stream, 16);
}

size_t mcr_attention_backward_pct_workspace_bytes(int64_t S, int64_t L) { return ab_workspace_bytes(S, L, VB_H, PB_E, 8); }

int mcr_attention_backward_pct(const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                               int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const char* who = "mcr_attention_backward_pct";
    MCR_REQUIRE(qkv && d_out && d_qkv, "%s: null pointer", who);
    MCR_REQUIRE(n_heads == VB_H && qk_dim == 8 * n_heads && v_dim == 32 * n_heads,
                "%s: 4 heads of widths 8 (q, k) and 32 (v) expected, got qk_dim %d, v_dim %d for %d heads", who, qk_dim, v_dim, n_heads);
    MCR_REQUIRE(S > 0 && L > 0 && (L == 16 || S <= 65535) && L <= (1 << 30) && S <= (1ll << 31), "%s: bad problem size S=%ld L=%ld (S <= 65535 unless L == 16)",
                who, (long)S, (long)L);
    MCR_REQUIRE(L != 16 || !lens, "%s: sequences of 16 tokens take no lens (every key takes part)", who);
    return ab_backward(who, qkv, ldq, d_out, ld_dout, d_qkv, ld_dqkv, S, L, n_heads, qk_dim, v_dim, lens, workspace, workspace_bytes, stream, 8);
}

}  // extern "C"
