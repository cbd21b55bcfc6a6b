// SconeVis backward for gfx950 (MI355X): gradients of SconeVis.forward (macarons/networks/SconeVis.py:121-162, default architecture)
// with respect to its 48 weight-table tensors, pts and view_harmonics, for the trainers' loss.backward() (pretrain_scone_vis.py:224,
// train_macarons.py:1159-1162).
//
// mcr_scone_vis_backward recomputes the forward of the fp32 network, keeping the residual stream at the four encoder boundaries and
// the pre-activations of the embedding and the head, then runs the backward in reverse order.  Each encoder's interior (LN1 output,
// qkv, attention output O and its log-sum-exp, post-attention residual, LN2 output, FF pre-activation and GELU) is rebuilt from its
// boundary just before that encoder's backward, in one region the three encoders share: one extra forward in all, one encoder's
// interior in memory.
//
// Building blocks (each behind its own C entry point, include/macarons_hip.h):
//   attention   flash-style: a stash-writing forward (O and LSE per (row, head)), then a query-major pass for dQ (and
//               delta = rowsum(dO * O)) and a key-major pass for dK, dV.  P = exp(S - LSE) is recomputed tile by tile; nothing
//               N x N is ever stored.  One lane owns one query (or key) row of one head; the 4 waves of a block share the row
//               block and split the other side's rows, their partial results meet in LDS in a fixed order.
//   linear      dZ = dY * GELU'(Z) (exact erf: Phi(z) + z phi(z)); dX = dZ W (written or added) on the forward's exact-fp32 MFMA GEMM
//               through a transposed weight copy; dW | db = dZ^T [X | 1] as a VALU split-K GEMM whose slabs are summed in a fixed order.
//   layernorm   per row mu, sigma recomputed (eps 1e-5); dx added into (or written to) the residual gradient; d_gamma | d_beta as
//               per-block column partials summed in a fixed order.
//   column max  the arg-max valid row of each column (ties: the lowest row, as torch.max(dim)) receives the column's gradient
//               summed over all rows.
// Numerics: fp32 throughout -- VALU FMA in the attention and weight-gradient kernels, the forward's exact-fp32 GEMM kernels
// (launch_linear routed to the fp32 MFMA kernel) in the recompute and the dX products.  The fp16 planes path is never taken, whatever the caller's variant: the result is the gradient of
// the fp32 network at the given inputs (on variants 6 and 7 too).  No float atomics: two calls give identical bits.
//
// PCTransformer backward (SconeOcc.py:45-130: SconeOcc's global transformer on one 2048-token sequence per cloud, its three local ones on
// B * Q sequences of 16 tokens): mcr_pc_transformer_backward, same scheme on the same launchers at E = 128.  The encoder's forward and
// backward (vb_encoder_fwd / vb_encoder_bwd) are shared with SconeVis and take the width; the attention kernels are compiled for the
// per-head widths (16, 64) and (8, 32).  Sequences of 16 tokens have a fused attention backward of their own (a16_bwd_kernel: one wave per
// sequence, nothing but d_qkv written) and are processed in chunks of PB_CHUNK16 sequences INSIDE the entry, their weight gradients
// summed in chunk order: the workspace holds one chunk whatever S is.  The tail's pooling has its own backward (pb_pool_bwd_kernel).
//
// SconeOcc backward (SconeOcc.py:250-347): mcr_scone_occ_backward, the network around the four PCTransformers behind one entry, given
// the neighbour indices.  The global transformer's forward runs once; then, cloud by cloud and chunk by chunk of its queries, the
// neighbourhoods are gathered as offsets (so_gather_kernel), the three local transformers, the x-embedding and the head run forward and
// backward on the chunk functions above (pb_chunk_forward / pb_chunk_backward) and the launchers of this file; the query's share of the
// offsets' gradient is so_dx_sub_kernel.  Weight gradients of the chunks behind the first are staged and added in chunk order, as are
// the chunks' column sums of the global features' gradient; the global transformer's backward runs last.  No gradient for the clouds.
//
// Ragged SconeOcc backward: mcr_scone_occ_backward_ragged, the gradient of J such calls of different sizes (the jobs of
// SconeOcc.forward_ragged) with the weight gradients summed over the jobs.  The neighbourhood offsets are an input, so everything but
// the global features is row-wise: the rows of all jobs are packed into full chunks that run the same chunk function
// (so_chunk_fwd_bwd).  The global transformer runs forward over the J padded sequences with their lengths (keys masked, pooling over
// the valid rows; so_pad_global_kernel first overwrites the padding), its features reach the rows through so_bcast_rows_kernel, their
// gradient comes back per job through so_seg_colsum_kernel, and its backward runs last, job by job in job order with lengths
// (pb_pool_bwd_lens_kernel hands exact zeros to the padded rows), the jobs behind the first through a staging area.
#include "nn_kernels.h"
#include "net_layout.h"
#include <algorithm>
#include <cmath>

namespace mcr {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int VB_E = 256, VB_F = 126, VB_H = 4;
// The attention kernels are compiled for two pairs of per-head widths <DQ (q, k), DV (v)>: (16, 64) SconeVis, (8, 32) PCTransformer
constexpr int AB_TILE = 32;                            // keys (queries) staged per wave and step
template <int DQ> constexpr float ab_scale() { return DQ == 16 ? 0.25f : 0.35355339059327379f; }   // 1 / sqrt(DQ), DQ = 16 or 8

__device__ __forceinline__ float gelu_f(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * __expf(-0.5f * z * z);
}

// ---- elementwise ------------------------------------------------------------------------------------------------------------------
// mode 0: Y = gelu(Z);  mode 1: Y *= gelu'(Z)
__global__ __launch_bounds__(256) void vb_gelu_kernel(const float* __restrict__ Z, long long ldz, float* Y, long long ldy, long long M,
                                                      int C, int mode) {
    const long long n = M * C;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long m = e / C;
        const int c = (int)(e - m * C);
        const float z = Z[m * ldz + c];
        float* y = Y + m * ldy + c;
        *y = mode == 0 ? gelu_f(z) : *y * gelu_d(z);
    }
}

void launch_gelu(hipStream_t s, const float* Z, int64_t ldz, float* Y, int64_t ldy, int64_t M, int C, int mode) {
    const long long n = M * C;
    if (n <= 0) return;
    hipLaunchKernelGGL(vb_gelu_kernel, dim3((unsigned)std::min<long long>(cdiv(n, 256), 8192)), dim3(256), 0, s, Z, (long long)ldz, Y,
                       (long long)ldy, (long long)M, C, mode);
}

// ---- weight-gradient GEMM: C[i*ldc + j] = sum_p A[i + p*ap] * B'(p, j),  B'(p, j) = B[p*bp + j] for j < nb, 1 for j == nb ------------
// 64 x 64 tiles, 256 threads of 4 x 4 outputs, depth-16 LDS steps.  blockIdx.z: the K slab [z * p_chunk, (z + 1) * p_chunk) whose sum
// goes to C + z * split_stride (split-K; the slabs are added in order by vb_reduce_kernel).  The ones column (nb < Nj) turns
// dW = dZ^T X into [dW | db] in one product.
__global__ __launch_bounds__(256) void vb_gemm_kernel(const float* __restrict__ A, long long ap, const float* __restrict__ B, long long bp,
                                                      int nb, float* C, long long ldc, long long split_stride, int Mi, int Nj, long long P,
                                                      long long p_chunk) {
    __shared__ alignas(16) float As[16][68];                      // (read as float4 below)
    __shared__ alignas(16) float Bs[16][68];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const long long pb = (long long)blockIdx.z * p_chunk, pe = std::min(P, pb + p_chunk);
    C += (long long)blockIdx.z * split_stride;
    f2 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][0] = acc[r][1] = f2{0.f, 0.f};
    for (long long p0 = pb; p0 < pe; p0 += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = t + 256 * r;
            const int pp = e >> 6, ii = e & 63;
            const long long p = p0 + pp;
            const int i = i0 + ii;
            As[pp][ii] = (p < pe && i < Mi) ? A[i + p * ap] : 0.f;
            const int jj = e & 63, qp = e >> 6;
            const long long q = p0 + qp;
            const int j = j0 + jj;
            Bs[qp][jj] = (q < pe && j < Nj) ? (j < nb ? B[q * bp + j] : 1.f) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
            const float4 b = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
            const f2 b01{b.x, b.y}, b23{b.z, b.w};
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f2 ar{av[r], av[r]};
                acc[r][0] = __builtin_elementwise_fma(ar, b01, acc[r][0]);
                acc[r][1] = __builtin_elementwise_fma(ar, b23, acc[r][1]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
        if (i >= Mi) continue;
        const float v[4] = {acc[r][0].x, acc[r][0].y, acc[r][1].x, acc[r][1].y};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx * 4 + c;
            if (j < Nj) C[(long long)i * ldc + j] = v[c];
        }
    }
}

// out[n*ldo + k] = sum_z part[z*stride + n*ldp + k] for k < kw, out_b[n] = the same at k == kw (when ldp > kw).  One block = 16
// outputs x 16 slab lanes; lane l adds slabs l, l + 16, ... and the 16 lane sums meet in a fixed tree: a fixed order throughout.
__global__ __launch_bounds__(256) void vb_reduce_kernel(const float* __restrict__ part, long long stride, int n_part, long long n_out,
                                                        int ldp, int kw, float* out, long long ldo, float* out_b) {
    __shared__ float red[16][17];
    const int o = threadIdx.x & 15, l = threadIdx.x >> 4;
    const long long e = blockIdx.x * 16ll + o;
    float acc = 0.f;
    if (e < n_out)
        for (int z = l; z < n_part; z += 16) acc += part[z * stride + e];
    red[l][o] = acc;
    __syncthreads();
    for (int w = 8; w > 0; w >>= 1) {
        if (l < w) red[l][o] += red[l + w][o];
        __syncthreads();
    }
    if (l == 0 && e < n_out) {
        const long long n = e / ldp;
        const int k = (int)(e - n * ldp);
        if (k < kw) {
            if (out) out[n * ldo + k] = red[0][o];
        } else if (out_b) {
            out_b[n] = red[0][o];
        }
    }
}

void launch_reduce(hipStream_t s, const float* part, long long stride, int n_part, long long n_out, int ldp, int kw, float* out, long long ldo,
                   float* out_b) {
    hipLaunchKernelGGL(vb_reduce_kernel, dim3((unsigned)cdiv(n_out, 16)), dim3(256), 0, s, part, stride, n_part, n_out, ldp, kw, out, ldo,
                       out_b);
}

// K slabs of the weight-gradient products: a function of the row count alone (determinism), at most 64 slabs
inline long long vb_slab_rows(int64_t M) { return std::max<long long>(256, cdiv(cdiv(M, 64), 16) * 16); }
inline long long vb_slabs(int64_t M) { return cdiv(M, vb_slab_rows(M)); }
inline size_t vb_gradw_floats(int64_t M, int N, int K) { return (size_t)vb_slabs(M) * N * (K + 1); }

// Wt[k*N + n] = W[n*ldw + k]   (n < N, k < K)
__global__ __launch_bounds__(256) void vb_transpose_kernel(const float* __restrict__ W, long long ldw, float* __restrict__ Wt, int N, int K) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= (long long)N * K) return;
    const int k = (int)(e / N), n = (int)(e - (long long)k * N);
    Wt[e] = W[n * ldw + k];
}

// dX[M, K] (= or +=) dZ[M, N] W[N, K]: the forward's exact-fp32 MFMA GEMM (launch_linear, routed on one row: never the split-precision
// kernels) on a transposed copy of W in wt (N * K floats); accumulate = the GEMM's residual operand, in place
void gemm_dx(hipStream_t s, const float* dZ, int64_t ldz, const float* W, int64_t ldw, float* dX, int64_t ldx, int64_t M, int N, int K,
             bool accumulate, float* wt) {
    hipLaunchKernelGGL(vb_transpose_kernel, dim3((unsigned)cdiv((int64_t)N * K, 256)), dim3(256), 0, s, W, (long long)ldw, wt, N, K);
    launch_linear(s, {dZ, ldz}, {wt, N}, {nullptr, ACT_NONE, {accumulate ? dX : nullptr, ldx}}, {dX, ldx}, M, K, N, /*route_rows=*/1);
}

// dW[N, K] = dZ^T X, db[N] = sum_rows dZ (either may be NULL); part: vb_gradw_floats(M, N, K) floats
void gemm_dw(hipStream_t s, const float* dZ, int64_t ldz, const float* X, int64_t ldx, int64_t M, int N, int K, float* dW, float* db,
             float* part) {
    if (!dW && !db) return;
    const long long rows = vb_slab_rows(M), slabs = vb_slabs(M);
    const long long stride = (long long)N * (K + 1);
    dim3 grid((unsigned)cdiv(N, 64), (unsigned)cdiv(K + 1, 64), (unsigned)slabs);
    hipLaunchKernelGGL(vb_gemm_kernel, grid, dim3(256), 0, s, dZ, (long long)ldz, X, (long long)ldx, K, part, (long long)(K + 1), stride, N,
                       K + 1, (long long)M, rows);
    launch_reduce(s, part, stride, (int)slabs, stride, K + 1, K, dW, K, db);
}

// ---- LayerNorm backward: one wave per row, 4 waves per block of `rows` rows ------------------------------------------------------------
// dX (= or +=) rstd (g - mean(g) - xhat mean(g xhat)), g = dY gamma;  part[blk][c][0 | 1] = sum over the block's rows of dY xhat | dY
template <int CPL>
__global__ __launch_bounds__(256) void vb_ln_bwd_kernel(const float* __restrict__ X, long long ldx, const float* __restrict__ gamma,
                                                        const float* __restrict__ dY, long long ldy, float* dX, long long ldd, int accumulate,
                                                        float* part, long long M, int rows) {
    constexpr int E = CPL * 64;
    __shared__ float red[3][2][E];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * rows, r1 = std::min<long long>(M, r0 + rows);
    const float inv_e = 1.0f / (float)E;
    float gam[CPL], pg[CPL], pb[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) { gam[j] = gamma[lane + 64 * j]; pg[j] = 0.f; pb[j] = 0.f; }
    for (long long r = r0 + w; r < r1; r += 4) {
        float x[CPL], dy[CPL];
        float sx = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) { x[j] = X[r * ldx + lane + 64 * j]; dy[j] = dY[r * ldy + lane + 64 * j]; sx += x[j]; }
        const float mean = wave_sum_all(sx) * inv_e;
        float sv = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) { const float d = x[j] - mean; sv = fmaf(d, d, sv); }
        const float rstd = 1.0f / sqrtf(wave_sum_all(sv) * inv_e + 1e-5f);
        float s1 = 0.f, s2 = 0.f, xh[CPL], g[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            xh[j] = (x[j] - mean) * rstd;
            g[j] = dy[j] * gam[j];
            s1 += g[j];
            s2 = fmaf(g[j], xh[j], s2);
            pg[j] = fmaf(dy[j], xh[j], pg[j]);
            pb[j] += dy[j];
        }
        s1 = wave_sum_all(s1) * inv_e;
        s2 = wave_sum_all(s2) * inv_e;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float dx = rstd * (g[j] - s1 - xh[j] * s2);
            float* o = dX + r * ldd + lane + 64 * j;
            *o = accumulate ? *o + dx : dx;
        }
    }
    if (w > 0)
#pragma unroll
        for (int j = 0; j < CPL; ++j) { red[w - 1][0][lane + 64 * j] = pg[j]; red[w - 1][1][lane + 64 * j] = pb[j]; }
    __syncthreads();
    if (w == 0) {
        float* pp = part + (long long)blockIdx.x * E * 2;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            pp[2 * c] = ((pg[j] + red[0][0][c]) + red[1][0][c]) + red[2][0][c];
            pp[2 * c + 1] = ((pb[j] + red[0][1][c]) + red[1][1][c]) + red[2][1][c];
        }
    }
}

inline int vb_ln_rows(int64_t M) { return (int)std::max<long long>(16, cdiv(cdiv(M, 256), 4) * 4); }
inline size_t vb_ln_part_floats(int64_t M, int E) { return (size_t)cdiv(M, vb_ln_rows(M)) * E * 2; }

void launch_ln_bwd(hipStream_t s, const float* X, int64_t ldx, const float* gamma, const float* dY, int64_t ldy, float* dX, int64_t ldd,
                   bool accumulate, float* d_gamma, float* d_beta, float* part, int64_t M, int E) {
    const int rows = vb_ln_rows(M);
    const long long blocks = cdiv(M, rows);
#define MCR_LNB(C) hipLaunchKernelGGL(vb_ln_bwd_kernel<C>, dim3((unsigned)blocks), dim3(256), 0, s, X, (long long)ldx, gamma, dY, (long long)ldy, \
                                      dX, (long long)ldd, (int)accumulate, part, (long long)M, rows)
    switch (E) {
        case 64: MCR_LNB(1); break;
        case 128: MCR_LNB(2); break;
        case 256: MCR_LNB(4); break;
        default: MCR_LNB(8); break;
    }
#undef MCR_LNB
    if (d_gamma || d_beta) launch_reduce(s, part, (long long)E * 2, (int)blocks, (long long)E * 2, 2, 1, d_gamma, 1, d_beta);
}

// ---- column-max backward ---------------------------------------------------------------------------------------------------------
// dX[(s*L + r*)*ldd + c] += sum_r dG[(s*L + r)*ldg + c], r* = the lowest valid row holding the column's max.  Block: 64 columns x 16
// row slices of one sequence; the slices meet in LDS in a fixed order.
__global__ __launch_bounds__(1024) void vb_colmax_bwd_kernel(const float* __restrict__ X, long long ldx, const float* __restrict__ dG,
                                                             long long ldg, float* dX, long long ldd, int L, int E,
                                                             const int* __restrict__ lens) {
    __shared__ float s_sum[16][64], s_max[16][64];
    __shared__ int s_arg[16][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const long long s = blockIdx.y;
    const int n_valid = lens ? std::min(L, std::max(1, lens[s])) : L;
    float sum = 0.f, best = -INFINITY;
    int arg = -1;
    if (c < E) {
        const float* g = dG + s * L * ldg + c;
#pragma unroll 8
        for (int r = sl; r < L; r += 16) sum += g[(long long)r * ldg];
        const float* x = X + s * L * ldx + c;
        for (int r = sl; r < n_valid; r += 16) {
            const float v = x[(long long)r * ldx];
            if (arg < 0 || v > best) { best = v; arg = r; }
        }
    }
    s_sum[sl][lane] = sum; s_max[sl][lane] = best; s_arg[sl][lane] = arg;
    __syncthreads();
    if (sl == 0 && c < E) {
        for (int k = 1; k < 16; ++k) {
            sum += s_sum[k][lane];
            const int a = s_arg[k][lane];
            const float v = s_max[k][lane];
            if (a >= 0 && (v > best || (v == best && a < arg))) { best = v; arg = a; }
        }
        float* o = dX + (s * L + arg) * ldd + c;
        *o += sum;
    }
}

void launch_colmax_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dG, int64_t ldg, float* dX, int64_t ldd, int64_t S, int L,
                       int E, const int* lens) {
    hipLaunchKernelGGL(vb_colmax_bwd_kernel, dim3((unsigned)cdiv(E, 64), (unsigned)S), dim3(1024), 0, s, X, (long long)ldx, dG, (long long)ldg,
                       dX, (long long)ldd, L, E, lens);
}

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
inline size_t ab_part_floats(int64_t S, int L, int H, int dq = 16, int dv = 64) {
    const int ns = ab_nsplit(S, L, H);
    return ns > 1 ? (size_t)ns * S * L * H * (dq + dv) : 0;   // (>= the forward's H * (dv + 2) and the dq parts' H * dq per row)
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

// dq: the per-head q / k width, 16 (v: 64) or 8 (v: 32)
void launch_attn_fwd(hipStream_t s, const float* qkv, int64_t ldq, float* O, int64_t ldo, float* lse, int64_t S, int L, int H, const int* lens,
                     float* part, int dq = 16) {
    if (dq == 16) launch_attn_fwd_t<16, 64>(s, qkv, ldq, O, ldo, lse, S, L, H, lens, part);
    else launch_attn_fwd_t<8, 32>(s, qkv, ldq, O, ldo, lse, S, L, H, lens, part);
}
void launch_attn_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* O, int64_t ldo, const float* lse, const float* dO,
                     int64_t lddo, float* delta, float* dqkv, int64_t lddq, int64_t S, int L, int H, const int* lens, float* part, int dq = 16) {
    if (dq == 16) launch_attn_bwd_t<16, 64>(s, qkv, ldq, O, ldo, lse, dO, lddo, delta, dqkv, lddq, S, L, H, lens, part);
    else launch_attn_bwd_t<8, 32>(s, qkv, ldq, O, ldo, lse, dO, lddo, delta, dqkv, lddq, S, L, H, lens, part);
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

// d_qkv of S sequences of 16 tokens, 4 heads of widths (8, 32); rows 16-byte aligned, leading dimensions multiples of 4
void launch_attn16_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* dO, int64_t lddo, float* dqkv, int64_t lddq, int64_t S) {
    hipLaunchKernelGGL(a16_bwd_kernel, dim3((unsigned)cdiv(S, A16_WAVES)), dim3(64 * A16_WAVES), 0, s, qkv, (long long)ldq, dO, (long long)lddo,
                       dqkv, (long long)lddq, (long long)S);
}

// ---- backward of the max || mean pooling over each sequence's rows (launch_pool_max_avg) -----------------------------------------------
// dX[(s*L + r)*ldd + c] = dY[s*ldy + E + c] / L + (r == r* ? dY[s*ldy + c] : 0), r* = the lowest row holding the column's max (as
// vb_colmax_bwd_kernel and torch.max(dim)).  Written, not accumulated.  Block: 64 columns x 16 row slices of one sequence.
__global__ __launch_bounds__(1024) void pb_pool_bwd_kernel(const float* __restrict__ X, long long ldx, const float* __restrict__ dY,
                                                           long long ldy, float* __restrict__ dX, long long ldd, int L, int E) {
    __shared__ float s_max[16][64];
    __shared__ int s_arg[16][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const long long s = blockIdx.x;
    float best = -INFINITY;
    int arg = -1;
    if (c < E) {
        const float* x = X + s * L * ldx + c;
        for (int r = sl; r < L; r += 16) {
            const float v = x[(long long)r * ldx];
            if (arg < 0 || v > best) { best = v; arg = r; }
        }
    }
    s_max[sl][lane] = best; s_arg[sl][lane] = arg;
    __syncthreads();
    if (c >= E) return;
    best = s_max[0][lane]; arg = s_arg[0][lane];
    for (int k = 1; k < 16; ++k) {
        const int a = s_arg[k][lane];
        const float v = s_max[k][lane];
        if (a >= 0 && (arg < 0 || v > best || (v == best && a < arg))) { best = v; arg = a; }
    }
    const float g_max = dY[s * ldy + c], g_avg = dY[s * ldy + E + c] / (float)L;
    float* o = dX + s * L * ldd + c;
    for (int r = sl; r < L; r += 16) o[(long long)r * ldd] = r == arg ? g_avg + g_max : g_avg;
}

// ... of padded sequences (launch_pool_max_avg with lens): with n = min(L, max(1, lens[s])) the arg-max runs over the first n rows (ties:
// the lowest row), the mean's share is dY / n, and rows >= n are written as exact zeros.  A kernel of its own: pb_pool_bwd_kernel stays
// what it is.
__global__ __launch_bounds__(1024) void pb_pool_bwd_lens_kernel(const float* __restrict__ X, long long ldx, const float* __restrict__ dY,
                                                                long long ldy, float* __restrict__ dX, long long ldd, int L, int E,
                                                                const int* __restrict__ lens) {
    __shared__ float s_max[16][64];
    __shared__ int s_arg[16][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const long long s = blockIdx.x;
    const int n = min(L, max(1, lens[s]));
    float best = -INFINITY;
    int arg = -1;
    if (c < E) {
        const float* x = X + s * L * ldx + c;
        for (int r = sl; r < n; r += 16) {
            const float v = x[(long long)r * ldx];
            if (arg < 0 || v > best) { best = v; arg = r; }
        }
    }
    s_max[sl][lane] = best; s_arg[sl][lane] = arg;
    __syncthreads();
    if (c >= E) return;
    best = s_max[0][lane]; arg = s_arg[0][lane];
    for (int k = 1; k < 16; ++k) {
        const int a = s_arg[k][lane];
        const float v = s_max[k][lane];
        if (a >= 0 && (arg < 0 || v > best || (v == best && a < arg))) { best = v; arg = a; }
    }
    const float g_max = dY[s * ldy + c], g_avg = dY[s * ldy + E + c] / (float)n;
    float* o = dX + s * L * ldd + c;
    for (int r = sl; r < L; r += 16) o[(long long)r * ldd] = r >= n ? 0.f : r == arg ? g_avg + g_max : g_avg;
}

// lens (optional, DEVICE int[S]): the valid rows of every sequence
void launch_pool_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ldd, int64_t S, int L, int E,
                     const int* lens = nullptr) {
    if (lens) {
        hipLaunchKernelGGL(pb_pool_bwd_lens_kernel, dim3((unsigned)S, (unsigned)cdiv(E, 64)), dim3(1024), 0, s, X, (long long)ldx, dY,
                           (long long)ldy, dX, (long long)ldd, L, E, lens);
        return;
    }
    hipLaunchKernelGGL(pb_pool_bwd_kernel, dim3((unsigned)S, (unsigned)cdiv(E, 64)), dim3(1024), 0, s, X, (long long)ldx, dY, (long long)ldy, dX,
                       (long long)ldd, L, E);
}

// ---- the network -------------------------------------------------------------------------------------------------------------------
// (the weight table and the arena of the workspace: net_layout.h)
// the encoder's interior, rebuilt from its input x: what its backward reads
struct VbInterior { float *h1, *qkv, *O, *lse, *xm, *h2, *z, *g, *part; };   // part: the attention's split scratch
constexpr int VB_W3 = 2 * 64 + VB_E;                             // packed q | k | v width

size_t vb_part_floats(int64_t T) {
    return std::max({vb_gradw_floats(T, 2 * VB_E, VB_E), vb_gradw_floats(T, VB_E, 2 * VB_E), vb_gradw_floats(T, VB_W3, VB_E),
                     vb_ln_part_floats(T, VB_E)});
}

// the fp32 GEMMs of the forward (launch_linear routed on one row: never the split-precision kernels)
void vb_linear(hipStream_t s, Rows X, const LinW& w, Rows R, RowsOut Y, int64_t T, int N, int K, int act) {
    launch_linear(s, X, {w.w, K}, {w.b, act, R}, Y, T, N, K, /*route_rows=*/1);
}

// An encoder of width E (256: SconeVis, 128: PCTransformer) with VB_H heads: q | k of E / 4 channels, v of E, packed rows of 3 E / 2.
// Sequences of 16 tokens at the PCTransformer's widths have a backward of their own (a16_bwd_kernel) that rebuilds the soft-max itself.
inline bool vb_fused16(int N, int E) { return N == 16 && E == 128; }

// x_out = Encoder(x) (x_out NULL: the interior for the backward, LSE included).  The boundary pass (x_out given) needs no LSE: it takes
// the forward's exact-fp32 MFMA attention (launch_attention, fp32 P V); so does the interior of 16-token sequences
void vb_encoder_fwd(hipStream_t s, const EncW& w, const float* x, float* x_out, const VbInterior& I, int64_t B, int N, const int* lens,
                    int E = VB_E) {
    const int64_t T = B * N;
    const int QK = E / 4, W3 = 2 * QK + E;
    launch_layernorm(s, x, E, w.n1g, w.n1b, I.h1, E, T, E);
    vb_linear(s, {I.h1, E}, w.qkv, {}, {I.qkv, W3}, T, W3, E, ACT_NONE);
    if (x_out || vb_fused16(N, E)) launch_attention(s, {I.qkv, W3}, {I.O, E}, B, N, VB_H, QK, E, lens, AttnSplit{}, /*pv_half=*/false);
    else launch_attn_fwd(s, I.qkv, W3, I.O, E, I.lse, B, N, VB_H, lens, I.part, QK / VB_H);
    vb_linear(s, {I.O, E}, w.out, {x, E}, {I.xm, E}, T, E, E, ACT_NONE);
    launch_layernorm(s, I.xm, E, w.n2g, w.n2b, I.h2, E, T, E);
    vb_linear(s, {I.h2, E}, w.ff1, {}, {I.z, 2 * E}, T, 2 * E, E, ACT_NONE);
    launch_gelu(s, I.z, 2 * E, I.g, 2 * E, T, 2 * E, 0);
    if (x_out) vb_linear(s, {I.g, 2 * E}, w.ff2, {I.xm, E}, {x_out, E}, T, E, 2 * E, ACT_NONE);
}

// The gradient buffers of an encoder's backward: dX [T, E] holds the gradient of the encoder's output on entry and of its input on return
struct VbGrads { float *dX, *dH, *dA, *dQKV, *delta, *part, *wt; };   // part / wt: weight-gradient slabs, transposed weight (gemm_dw / gemm_dx)

// Backward of one encoder (Attention.py:278-300) whose interior I was rebuilt from its input x.  dw: where the gradients of the encoder's
// ENC_NW table entries go (NULL: none wanted)
void vb_encoder_bwd(hipStream_t s, const EncW& we, float* const* dw, const float* x, const VbInterior& I, const VbGrads& G, int64_t B, int N,
                    const int* lens, int E = VB_E) {
    const int64_t T = B * N;
    const int QK = E / 4, W3 = 2 * QK + E;
    float *dX = G.dX, *dH = G.dH, *dA = G.dA, *dQKV = G.dQKV, *part = G.part, *wt = G.wt;
    auto DW = [&](int slot) { return dw ? dw[slot] : nullptr; };
    gemm_dw(s, dX, E, I.g, 2 * E, T, E, 2 * E, DW(ENC_FF2 + LIN_W), DW(ENC_FF2 + LIN_B), part);          // ff2
    gemm_dx(s, dX, E, we.ff2.w, 2 * E, dH, 2 * E, T, E, 2 * E, false, wt);
    launch_gelu(s, I.z, 2 * E, dH, 2 * E, T, 2 * E, 1);                      // ff1
    gemm_dw(s, dH, 2 * E, I.h2, E, T, 2 * E, E, DW(ENC_FF1 + LIN_W), DW(ENC_FF1 + LIN_B), part);
    gemm_dx(s, dH, 2 * E, we.ff1.w, E, dA, E, T, 2 * E, E, false, wt);
    launch_ln_bwd(s, I.xm, E, we.n2g, dA, E, dX, E, true, DW(ENC_N2G), DW(ENC_N2B), part, T, E);   // norm2 (+ residual)
    gemm_dw(s, dX, E, I.O, E, T, E, E, DW(ENC_OUT + LIN_W), DW(ENC_OUT + LIN_B), part);        // out
    gemm_dx(s, dX, E, we.out.w, E, dA, E, T, E, E, false, wt);
    if (vb_fused16(N, E)) {
        if (lens) { refuse("vb_encoder_bwd: 16-token sequences take no lens (every key takes part)"); return; }
        launch_attn16_bwd(s, I.qkv, W3, dA, E, dQKV, W3, B);
    }
    else launch_attn_bwd(s, I.qkv, W3, I.O, E, I.lse, dA, E, G.delta, dQKV, W3, B, N, VB_H, lens, I.part, QK / VB_H);
    gemm_dw(s, dQKV, W3, I.h1, E, T, W3, E, DW(ENC_QKV + LIN_W), DW(ENC_QKV + LIN_B), part);   // qkv
    gemm_dx(s, dQKV, W3, we.qkv.w, E, dA, E, T, W3, E, false, wt);
    launch_ln_bwd(s, x, E, we.n1g, dA, E, dX, E, true, DW(ENC_N1G), DW(ENC_N1B), part, T, E);   // norm1 (+ residual)
}

// The workspace of mcr_scone_vis_backward over T = B * N tokens
struct VbScratch {
    float* X[VIS_N_ENC + 1];                               // the residual stream at the encoder boundaries
    float *z1, *g1;                                        // the embedding's pre-activation and its GELU
    float *hn, *zf1, *c2, *zf2, *gf2;                      // head: final LayerNorm, fc1 pre-activation, [GELU(fc1) | harmonics], fc2 pre-activation, its GELU
    VbInterior I;                                          // one encoder's interior (the three share it)
    float *dX, *dH, *dA, *dQKV, *delta;                    // gradients
    float *part, *wt;                                      // slabs / column partials of the weight gradients; transposed weight (dX products)
};
VbScratch carve_vb(Arena& a, int64_t B, int64_t N) {
    const int64_t T = B * N;
    VbScratch w;
    for (float*& x : w.X) x = a.f(T * VB_E);
    w.z1 = a.f(T * VB_F); w.g1 = a.f(T * VB_F);
    w.hn = a.f(T * VB_E); w.zf1 = a.f(T * 192); w.c2 = a.f(T * VB_E); w.zf2 = a.f(T * 128); w.gf2 = a.f(T * 128);
    VbInterior& I = w.I;
    I.h1 = a.f(T * VB_E); I.qkv = a.f(T * VB_W3); I.O = a.f(T * VB_E); I.lse = a.f(T * VB_H);
    I.xm = a.f(T * VB_E); I.h2 = a.f(T * VB_E); I.z = a.f(T * 2 * VB_E); I.g = a.f(T * 2 * VB_E);
    w.dX = a.f(T * VB_E); w.dH = a.f(T * 2 * VB_E); w.dA = a.f(T * VB_E); w.dQKV = a.f(T * VB_W3); w.delta = a.f(T * VB_H);
    w.part = a.f(vb_part_floats(T));
    w.wt = a.f((size_t)2 * VB_E * VB_E);
    I.part = a.f(ab_part_floats(B, (int)N, VB_H));
    return w;
}
constexpr size_t VB_WS_SLACK = 4096, VB_BLOCK_WS_SLACK = 1024;

// ... and of the three building blocks
struct AttnBwdScratch { float *O, *lse, *delta, *part; };
AttnBwdScratch carve_attention_backward(Arena& a, int64_t S, int64_t L, int n_heads, int v_dim) {
    const int64_t T = S * L;
    AttnBwdScratch w;
    w.O = a.f(T * v_dim);
    w.lse = a.f(T * n_heads);
    w.delta = a.f(T * n_heads);
    w.part = a.f(ab_part_floats(S, (int)L, n_heads));
    return w;
}
struct LinBwdScratch { float *dz, *part, *wt; };
LinBwdScratch carve_linear_backward(Arena& a, int64_t M, int N, int K) {
    LinBwdScratch w;
    w.dz = a.f((size_t)M * N);
    w.part = a.f(vb_gradw_floats(M, N, K));
    w.wt = a.f((size_t)N * K);
    return w;
}
float* carve_layernorm_backward(Arena& a, int64_t M, int E) { return a.f(vb_ln_part_floats(M, E)); }

// ---- PCTransformer (SconeOcc.py:45-130): E = 128, 2 encoders, 4 heads of widths (8, 32) ---------------------------------------------------
constexpr int PB_E = 128, PB_F = 125, PB_W3 = 2 * 32 + PB_E;        // PB_F: the embedding's inner width (E - 3: the raw points fill the row)
// Sequences of 16 tokens arrive by the ten thousand (B * Q neighbourhoods): they are processed in chunks of PB_CHUNK16 sequences, a
// function of (S, L) alone, so the workspace does not grow with S; the chunks' weight gradients are summed in chunk order.
constexpr int64_t PB_CHUNK16 = 2048;
inline int64_t pb_chunk(int64_t S, int64_t L) { return L == 16 ? std::min(S, PB_CHUNK16) : S; }

// floats of the table entry `slot` (half = feature_dim / 2)
inline int pb_slot_floats(int slot, int half) {
    if (slot == PCT_L1 + LIN_W) return PB_F * 3;
    if (slot == PCT_L2 + LIN_W) return PB_F * PB_F;
    if (slot == PCT_L1 + LIN_B || slot == PCT_L2 + LIN_B) return PB_F;
    if (slot == PCT_LIN0 + LIN_W) return half * PB_E;
    if (slot == PCT_LIN0 + LIN_B) return half;
    if (slot >= PCT_ENC && slot < PCT_NG) {
        switch ((slot - PCT_ENC) % ENC_NW) {
            case ENC_QKV + LIN_W: return PB_W3 * PB_E;
            case ENC_QKV + LIN_B: return PB_W3;
            case ENC_OUT + LIN_W: return PB_E * PB_E;
            case ENC_FF1 + LIN_W: case ENC_FF2 + LIN_W: return 2 * PB_E * PB_E;
            case ENC_FF1 + LIN_B: return 2 * PB_E;
            default: return PB_E;                                   // norm1, norm2, out.bias, ff2.bias
        }
    }
    return PB_E;                                                    // the final norm
}
// a later chunk's weight gradients: one contiguous staging area, cut in table order
struct PbSlots { float* dst[PCT_NW]; int off[PCT_NW + 1]; };
__global__ __launch_bounds__(256) void pb_add_slots_kernel(PbSlots t, const float* __restrict__ stage) {
    const int slot = blockIdx.y, n = t.off[slot + 1] - t.off[slot];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) t.dst[slot][e] += stage[t.off[slot] + e];
}

// The workspace of mcr_pc_transformer_backward: one chunk of Sc sequences (T = Sc * L tokens)
struct PbScratch {
    float* X[PCT_N_ENC + 1];                               // the residual stream at the encoder boundaries
    float *z1, *g1;                                        // the embedding's pre-activation and its GELU
    float *hn, *y0;                                        // tail: final LayerNorm, linear0's output (what the pooling reads)
    VbInterior I;                                          // one encoder's interior (the two share it)
    VbGrads G;
    float* stage;                                          // weight gradients of the chunks behind the first
};
// one chunk of Sc sequences; with_stage: the staging area of the chunks behind the first
PbScratch carve_pb_chunk(Arena& a, int64_t Sc, int64_t L, int half, bool with_stage) {
    const int64_t T = Sc * L;
    PbScratch w;
    for (float*& x : w.X) x = a.f(T * PB_E);
    w.z1 = a.f(T * PB_F); w.g1 = a.f(T * PB_F);
    w.hn = a.f(T * PB_E); w.y0 = a.f(T * half);
    VbInterior& I = w.I;
    const bool stash = !vb_fused16((int)L, PB_E);           // the 16-token attention backward keeps LSE, delta and parts in the wave
    I.h1 = a.f(T * PB_E); I.qkv = a.f(T * PB_W3); I.O = a.f(T * PB_E); I.lse = a.f(stash ? T * VB_H : 0);
    I.xm = a.f(T * PB_E); I.h2 = a.f(T * PB_E); I.z = a.f(T * 2 * PB_E); I.g = a.f(T * 2 * PB_E);
    I.part = a.f(stash ? ab_part_floats(Sc, (int)L, VB_H, 8, 32) : 0);
    VbGrads& G = w.G;
    G.dX = a.f(T * PB_E); G.dH = a.f(T * 2 * PB_E); G.dA = a.f(T * PB_E); G.dQKV = a.f(T * PB_W3); G.delta = a.f(stash ? T * VB_H : 0);
    G.part = a.f(std::max({vb_gradw_floats(T, 2 * PB_E, PB_E), vb_gradw_floats(T, PB_E, 2 * PB_E), vb_gradw_floats(T, PB_W3, PB_E),
                           vb_gradw_floats(T, half, PB_E), vb_gradw_floats(T, PB_F, PB_F), vb_ln_part_floats(T, PB_E)}));
    G.wt = a.f((size_t)2 * PB_E * PB_E);
    size_t n_stage = 0;
    if (with_stage)
        for (int i = 0; i < PCT_NW; ++i) n_stage += pb_slot_floats(i, half);
    w.stage = a.f(n_stage);
    return w;
}
PbScratch carve_pb(Arena& a, int64_t S, int64_t L, int half) {
    const int64_t Sc = pb_chunk(S, L);
    return carve_pb_chunk(a, Sc, L, half, Sc < S);
}
AttnBwdScratch carve_attention_backward_pct(Arena& a, int64_t S, int64_t L) {
    AttnBwdScratch w{};
    if (L == 16) return w;                                 // (the 16-token kernel keeps everything in the wave)
    const int64_t T = S * L;
    w.O = a.f(T * PB_E);
    w.lse = a.f(T * VB_H);
    w.delta = a.f(T * VB_H);
    w.part = a.f(ab_part_floats(S, (int)L, VB_H, 8, 32));
    return w;
}

// Forward of the fp32 network over one chunk of Sc sequences: boundaries X0..X2, the embedding's pre-activation, the tail up to
// linear0's output ws.y0 (what the pooling reads)
// lens (optional, DEVICE int[Sc]): padded sequences -- the keys of sequence i are its first min(L, max(1, lens[i])) rows
void pb_chunk_forward(hipStream_t s, const PctW& w, const float* pc, int64_t Sc, int L, int half, const PbScratch& ws,
                      const int* lens = nullptr) {
    const int64_t T = Sc * L;
    float* const* X = ws.X;
    const VbInterior& I = ws.I;
    vb_linear(s, {pc, 3}, w.l1, {}, {ws.z1, PB_F}, T, PB_F, 3, ACT_NONE);
    launch_gelu(s, ws.z1, PB_F, ws.g1, PB_F, T, PB_F, 0);
    vb_linear(s, {ws.g1, PB_F}, w.l2, {}, {X[0], PB_E}, T, PB_F, PB_F, ACT_NONE);
    launch_copy2d(s, pc, 3, X[0] + PB_F, PB_E, T, 3);
    for (int e = 0; e < PCT_N_ENC; ++e) vb_encoder_fwd(s, w.enc[e], X[e], X[e + 1], I, Sc, L, lens, PB_E);
    launch_layernorm(s, X[PCT_N_ENC], PB_E, w.ng, w.nb, ws.hn, PB_E, T, PB_E);
    vb_linear(s, {ws.hn, PB_E}, w.lin0, {}, {ws.y0, half}, T, half, PB_E, ACT_NONE);
}

// One chunk: Sc sequences from pc / d_feat on; dw = where the table's gradients go (NULL: none), d_pc (optional) this chunk's rows;
// ld_feat: the leading dimension of d_feat (0: 2 * half, dense rows); forward_done: ws still holds pb_chunk_forward's results for this
// very chunk (nothing has written it since), so the forward is not run again; lens: as pb_chunk_forward, the pooling's too (padded
// rows then receive exact zeros from the pooling's backward and hand exact zeros on: nothing of them reaches a gradient)
void pb_chunk_backward(hipStream_t s, const PctW& w, const float* pc, const float* d_feat, int64_t Sc, int L, int half, float* const* dw,
                       float* d_pc, const PbScratch& ws, int64_t ld_feat = 0, bool forward_done = false, const int* lens = nullptr) {
    const int64_t T = Sc * L;
    float* const* X = ws.X;
    const VbInterior& I = ws.I;
    const VbGrads& G = ws.G;
    auto DW = [&](int slot) { return dw ? dw[slot] : nullptr; };
    if (!forward_done) pb_chunk_forward(s, w, pc, Sc, L, half, ws, lens);
    // ---- tail (SconeOcc.py:119-126), backwards: pooling, linear0, norm
    launch_pool_bwd(s, ws.y0, half, d_feat, ld_feat > 0 ? ld_feat : 2 * half, G.dH, half, Sc, L, half, lens);
    gemm_dw(s, G.dH, half, ws.hn, PB_E, T, half, PB_E, DW(PCT_LIN0 + LIN_W), DW(PCT_LIN0 + LIN_B), G.part);
    gemm_dx(s, G.dH, half, w.lin0.w, PB_E, G.dA, PB_E, T, half, PB_E, false, G.wt);
    launch_ln_bwd(s, X[PCT_N_ENC], PB_E, w.ng, G.dA, PB_E, G.dX, PB_E, false, DW(PCT_NG), DW(PCT_NB), G.part, T, PB_E);
    // ---- encoders, last to first
    for (int e = PCT_N_ENC - 1; e >= 0; --e) {
        vb_encoder_fwd(s, w.enc[e], X[e], nullptr, I, Sc, L, lens, PB_E);
        vb_encoder_bwd(s, w.enc[e], dw ? dw + PCT_ENC + ENC_NW * e : nullptr, X[e], I, G, Sc, L, lens, PB_E);
    }
    // ---- embedding (Attention.py:98-128): [linear2(GELU(linear1(pc))) | pc]
    gemm_dw(s, G.dX, PB_E, ws.g1, PB_F, T, PB_F, PB_F, DW(PCT_L2 + LIN_W), DW(PCT_L2 + LIN_B), G.part);
    gemm_dx(s, G.dX, PB_E, w.l2.w, PB_F, G.dH, PB_F, T, PB_F, PB_F, false, G.wt);
    launch_gelu(s, ws.z1, PB_F, G.dH, PB_F, T, PB_F, 1);
    gemm_dw(s, G.dH, PB_F, pc, 3, T, PB_F, 3, DW(PCT_L1 + LIN_W), DW(PCT_L1 + LIN_B), G.part);
    if (d_pc) {
        launch_copy2d(s, G.dX + PB_F, PB_E, d_pc, 3, T, 3);
        gemm_dx(s, G.dH, PB_F, w.l1.w, 3, d_pc, 3, T, PB_F, 3, true, G.wt);
    }
}


// ---- SconeOcc (SconeOcc.py:250-347): the network around the four PCTransformers -------------------------------------------------------
constexpr int SO_K = 16;                                            // neighbours per query and scale
constexpr int SO_G = 512, SO_LF = 256, SO_XE = 512, SO_VH = 64;     // widths of the head's input: global | 3 x local | x-embedding | harmonics
constexpr int SO_LOC = SO_G, SO_XCOL = SO_LOC + 3 * SO_LF, SO_VCOL = SO_XCOL + SO_XE, SO_H = SO_VCOL + SO_VH;   // its columns (1856 in all)
constexpr int SO_L1 = 512, SO_L2 = 256;                             // the head's hidden widths
constexpr int SO_HEAD_NW = 6 * LIN_NW;                              // x_embedding.linear{1,2,3}, linear{1,2,3}: the table from OCC_XE on
static_assert(SO_H == 1856 && OCC_LIN == OCC_XE + 3 * LIN_NW && SO_HEAD_NW <= PCT_NW, "SconeOcc head layout");

// floats of the table entry OCC_XE + slot
inline int so_head_slot_floats(int slot) {
    constexpr int n[6] = {SO_XE / 4, SO_XE / 2, SO_XE, SO_L1, SO_L2, 1}, k[6] = {3, SO_XE / 4, SO_XE / 2, SO_H, SO_L1, SO_L2};
    return slot % LIN_NW == LIN_W ? n[slot / LIN_NW] * k[slot / LIN_NW] : n[slot / LIN_NW];
}

// off[(r*16 + j)*3 + c] = pc[idx[r*16 + j]*3 + c] - x[r*3 + c]: the neighbourhoods of `rows` queries of one cloud of M points, as offsets
// (SconeOcc.py:296-300; the fp32 subtraction torch performs).  One thread per (query, neighbour); an index outside the cloud is clamped
// into it (never an access out of bounds).
__global__ __launch_bounds__(256) void so_gather_kernel(const float* __restrict__ pc, long long M, const long long* __restrict__ idx,
                                                        const float* __restrict__ x, float* __restrict__ off, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * SO_K) return;
    const long long r = e / SO_K;
    const long long i = min(max(idx[e], 0ll), M - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) off[e * 3 + c] = pc[i * 3 + c] - x[r * 3 + c];
}

// d_x[r*3 + c] -= sum_j d_off[(r*16 + j)*3 + c], j ascending: the query's share of its neighbourhood's offsets.  One thread per (query,
// channel) owns its output: no atomics.
__global__ __launch_bounds__(256) void so_dx_sub_kernel(const float* __restrict__ d_off, float* __restrict__ d_x, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * 3) return;
    const long long r = e / 3;
    const int c = (int)(e - r * 3);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < SO_K; ++j) acc += d_off[(r * SO_K + j) * 3 + c];
    d_x[e] -= acc;
}

void launch_so_gather(hipStream_t s, const float* pc, int64_t M, const int64_t* idx, const float* x, float* off, int64_t rows) {
    hipLaunchKernelGGL(so_gather_kernel, dim3((unsigned)cdiv(rows * SO_K, 256)), dim3(256), 0, s, pc, (long long)M, (const long long*)idx, x, off,
                       (long long)rows);
}
void launch_so_dx_sub(hipStream_t s, const float* d_off, float* d_x, int64_t rows) {
    hipLaunchKernelGGL(so_dx_sub_kernel, dim3((unsigned)cdiv(rows * 3, 256)), dim3(256), 0, s, d_off, d_x, (long long)rows);
}

inline int64_t so_chunk(int64_t Q, int64_t q_chunk) { return std::min<int64_t>(q_chunk > 0 ? q_chunk : PB_CHUNK16, Q); }

// The workspace of mcr_scone_occ_backward: what outlives a chunk (the global features and their gradient), then one chunk of Qc queries
// OVER the global transformer's scratch -- the two are never alive together (the global forward runs first, its backward last).
struct SoScratch {
    float *gfeat, *dG, *gtmp;                              // [B, 512] global features and their gradient; one chunk's partial of a row of it
    float *off[3], *d_off;                                 // the chunk's neighbourhoods [Qc, 16, 3] per scale; the gradient of one of them
    float *ze1, *ge1, *ze2, *ge2, *ze3;                    // x-embedding: pre-activations and GELUs
    float *h, *z1, *g1, *z2, *g2, *z3;                     // head: input [Qc, 1856], pre-activations and GELUs
    float *dH, *d1, *d2, *dz3;                             // gradients: head input; 512- and 256-wide layers (the x-embedding's 128 / 256 too); output
    float *part, *wt;                                      // weight-gradient slabs; transposed weight
    float* stage;                                          // weight gradients of the chunks behind the first: 3 PCT tables, then the head's
    PbScratch local[3];                                    // one 16-token chunk per scale: each keeps what its forward leaves (boundaries, embedding
                                                           // and tail), the three share the encoder interior and the gradient buffers
    PbScratch global;                                      // B sequences of Lg tokens
};
inline size_t so_stage_pct_floats() {
    size_t n = 0;
    for (int i = 0; i < PCT_NW; ++i) n += pb_slot_floats(i, SO_LF / 2);
    return n;
}
// one chunk of Qc queries (everything of SoScratch but what outlives a chunk and the global transformer's scratch)
void carve_so_chunk(Arena& c, SoScratch& w, int64_t Qc) {
    for (float*& o : w.off) o = c.f(Qc * SO_K * 3);
    w.d_off = c.f(Qc * SO_K * 3);
    w.ze1 = c.f(Qc * (SO_XE / 4)); w.ge1 = c.f(Qc * (SO_XE / 4)); w.ze2 = c.f(Qc * (SO_XE / 2)); w.ge2 = c.f(Qc * (SO_XE / 2));
    w.ze3 = c.f(Qc * SO_XE);
    w.h = c.f(Qc * SO_H); w.z1 = c.f(Qc * SO_L1); w.g1 = c.f(Qc * SO_L1); w.z2 = c.f(Qc * SO_L2); w.g2 = c.f(Qc * SO_L2); w.z3 = c.f(Qc);
    w.dH = c.f(Qc * SO_H); w.d1 = c.f(Qc * SO_L1); w.d2 = c.f(Qc * SO_L2); w.dz3 = c.f(Qc);
    w.part = c.f(std::max({vb_gradw_floats(Qc, SO_L1, SO_H), vb_gradw_floats(Qc, SO_L2, SO_L1), vb_gradw_floats(Qc, 1, SO_L2),
                           vb_gradw_floats(Qc, SO_XE, SO_XE / 2), vb_gradw_floats(Qc, SO_XE / 2, SO_XE / 4), vb_gradw_floats(Qc, SO_XE / 4, 3)}));
    w.wt = c.f((size_t)SO_L1 * SO_H);
    size_t n_stage = 3 * so_stage_pct_floats();
    for (int i = 0; i < SO_HEAD_NW; ++i) n_stage += so_head_slot_floats(i);
    w.stage = c.f(n_stage);
    w.local[0] = carve_pb_chunk(c, Qc, SO_K, SO_LF / 2, false);
    for (int i = 1; i < 3; ++i) {
        PbScratch& l = w.local[i];
        const int64_t T = Qc * SO_K;
        l = w.local[0];
        for (float*& x : l.X) x = c.f(T * PB_E);
        l.z1 = c.f(T * PB_F); l.g1 = c.f(T * PB_F);
        l.hn = c.f(T * PB_E); l.y0 = c.f(T * (SO_LF / 2));
    }
}
SoScratch carve_so(Arena& a, int64_t B, int64_t Qc, int64_t Lg) {
    SoScratch w;
    w.gfeat = a.f(B * SO_G); w.dG = a.f(B * SO_G); w.gtmp = a.f(SO_G);
    Arena c = a.rest(), g = a.rest();
    carve_so_chunk(c, w, Qc);
    w.global = carve_pb_chunk(g, B, Lg, SO_G / 2, false);
    a.off += std::max(c.off, g.off);
    return w;
}

// The workspace of mcr_scone_occ_backward_ragged: as SoScratch over J jobs (so.global: the J padded sequences' forward), plus the padded
// sequences with their padding overwritten, and ONE sequence's scratch for the global transformer's backward, which runs job by job
// (the jobs behind the first through a staging area of their own)
struct SoRaggedScratch {
    SoScratch so;
    float* pcg;                                            // [J, Lg, 3]: pc_global, rows >= the length = the sequence's row 0
    PbScratch global1;                                     // one sequence of Lg tokens (with its staging area)
};
SoRaggedScratch carve_so_ragged(Arena& a, int64_t J, int64_t Qc, int64_t Lg) {
    SoRaggedScratch r;
    SoScratch& w = r.so;
    w.gfeat = a.f(J * SO_G); w.dG = a.f(J * SO_G); w.gtmp = nullptr;
    r.pcg = a.f(J * Lg * 3);
    Arena c = a.rest(), g = a.rest(), g1 = a.rest();
    carve_so_chunk(c, w, Qc);
    w.global = carve_pb_chunk(g, J, Lg, SO_G / 2, false);
    r.global1 = carve_pb_chunk(g1, 1, Lg, SO_G / 2, true);
    a.off += std::max({c.off, g.off, g1.off});
    return r;
}

// ---- the ragged pass: rows of J jobs packed into chunks -------------------------------------------------------------------------------
// dst[(j*L + r)*3 + c] = src[(j*L + (r < n ? r : 0))*3 + c], n = min(L, max(1, lens[j])): the padded sequences with their padding
// overwritten by a valid row.  The forward masks the padded keys, but the weight-gradient products of the backward multiply every row's
// (zero) gradient with what the row holds: 0 x NaN would be NaN.  One thread per (row, channel).
__global__ __launch_bounds__(256) void so_pad_global_kernel(const float* __restrict__ src, const int* __restrict__ lens,
                                                            float* __restrict__ dst, long long J, int L) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= J * L * 3) return;
    const long long row = e / 3;
    const int c = (int)(e - row * 3);
    const long long j = row / L;
    const int r = (int)(row - j * L);
    const int n = min(L, max(1, lens[j]));
    dst[e] = src[(j * L + (r < n ? r : 0)) * 3 + c];
}

// h[r*ldh + c] = gfeat[row_job[r]*512 + c] (c < 512): every row's job's global features into the head's input.  One thread per (row,
// column), consecutive threads on consecutive columns; a job outside [0, J) is clamped into it (never an access out of bounds).
__global__ __launch_bounds__(256) void so_bcast_rows_kernel(const float* __restrict__ gfeat, const int* __restrict__ row_job, long long J,
                                                            float* __restrict__ h, long long ldh, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * SO_G) return;
    const long long r = e / SO_G;
    const int c = (int)(e - r * SO_G);
    const long long j = min(max((long long)row_job[r], 0ll), J - 1);
    h[r * ldh + c] = gfeat[j * SO_G + c];
}

// dG[j*512 + c] += sum of dH[(r - r0)*ldh + c] over the rows r of job j inside the chunk [r0, r0 + rows), r ascending; job j = rows
// [job_rows[j], job_rows[j + 1]) (clamped into the chunk: never an access out of bounds).  One thread owns each (j, c): no atomics, and
// the chunks run one behind the other on the stream, so the sum has one order.  A job without rows in the chunk is left alone.
__global__ __launch_bounds__(256) void so_seg_colsum_kernel(const float* __restrict__ dH, long long ldh, const long long* __restrict__ job_rows,
                                                            long long J, long long r0, long long rows, float* __restrict__ dG) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= J * SO_G) return;
    const long long j = e / SO_G;
    const int c = (int)(e - j * SO_G);
    const long long lo = min(max(job_rows[j], r0), r0 + rows) - r0, hi = min(max(job_rows[j + 1], r0), r0 + rows) - r0;
    if (lo >= hi) return;
    float acc = 0.f;
#pragma unroll 8
    for (long long r = lo; r < hi; ++r) acc += dH[r * ldh + c];
    dG[e] += acc;
}

// How a chunk's rows meet the global features: all of one cloud (row_job NULL: gfeat / dG are that cloud's rows of 512, and the cloud's
// first chunk writes dG where the later ones add), or every row with its job (gfeat / dG [J, 512]; row_job: the chunk's slice, r0: its
// first row)
struct SoGlobalRows {
    const float* gfeat; float* dG; float* gtmp; bool first_of_cloud;
    const int* row_job; const long long* job_rows; int64_t J, r0;
};

// the chunks behind the first leave their weight gradients in the staging area, cut in table order, and are added in chunk order
struct SoStage {
    float* tab[OCC_NW] = {};
    PbSlots local[3] = {}, head{};
    const float* stage_local[3] = {};
    const float* stage_head = nullptr;
};
void so_stage_init(SoStage& st, float* const* d_weights, float* stage) {
    const size_t n_pct = so_stage_pct_floats();
    for (int i = 0; i < 3; ++i) {
        st.stage_local[i] = stage + i * n_pct;
        for (int k = 0; k < PCT_NW; ++k) {
            st.local[i].dst[k] = d_weights[OCC_LOCAL + i * PCT_NW + k];
            st.local[i].off[k + 1] = st.local[i].off[k] + pb_slot_floats(k, SO_LF / 2);
            st.tab[OCC_LOCAL + i * PCT_NW + k] = stage + i * n_pct + st.local[i].off[k];
        }
    }
    st.stage_head = stage + 3 * n_pct;
    for (int k = 0; k < SO_HEAD_NW; ++k) {
        st.head.dst[k] = d_weights[OCC_XE + k];
        st.head.off[k + 1] = st.head.off[k] + so_head_slot_floats(k);
        st.tab[OCC_XE + k] = stage + 3 * n_pct + st.head.off[k];
    }
}
void so_stage_add(hipStream_t s, const SoStage& st) {
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(pb_add_slots_kernel, dim3(64, PCT_NW), dim3(256), 0, s, st.local[i], st.stage_local[i]);
    hipLaunchKernelGGL(pb_add_slots_kernel, dim3(64, SO_HEAD_NW), dim3(256), 0, s, st.head, st.stage_head);
}

// One chunk of n rows, forward and backward, given its neighbourhoods as offsets off[i] [n, 16, 3]: (b) the local features, (c) the
// x-embedding, (d) the head, then (e) - (h) their backward.  xc / vhc / d_out_c / dxc / dvhc: the chunk's rows of the operands (dxc, dvhc
// may be NULL); dw: where this chunk's weight gradients go (NULL: none wanted); deep: anything below the head's input wanted
void so_chunk_fwd_bwd(hipStream_t s, const OccW& w, const SoScratch& ws, const float* const* off, const float* xc, const float* vhc,
                      const float* d_out_c, int64_t n, float* const* dw, float* dxc, float* dvhc, bool deep, const SoGlobalRows& g) {
    float *part = ws.part, *wt = ws.wt;
    auto DW = [&](int slot) { return dw ? dw[slot] : nullptr; };
    // (b) the local features, straight into the head's input
    for (int i = 0; i < 3; ++i) {
        pb_chunk_forward(s, w.local[i], off[i], n, SO_K, SO_LF / 2, ws.local[i]);
        launch_pool_max_avg(s, ws.local[i].y0, SO_LF / 2, ws.h + SO_LOC + i * SO_LF, SO_H, n, SO_K, SO_LF / 2);
    }
    // (c) the x-embedding (SconeOcc.py:7-42)
    vb_linear(s, {xc, 3}, w.xe1, {}, {ws.ze1, SO_XE / 4}, n, SO_XE / 4, 3, ACT_NONE);
    launch_gelu(s, ws.ze1, SO_XE / 4, ws.ge1, SO_XE / 4, n, SO_XE / 4, 0);
    vb_linear(s, {ws.ge1, SO_XE / 4}, w.xe2, {}, {ws.ze2, SO_XE / 2}, n, SO_XE / 2, SO_XE / 4, ACT_NONE);
    launch_gelu(s, ws.ze2, SO_XE / 2, ws.ge2, SO_XE / 2, n, SO_XE / 2, 0);
    vb_linear(s, {ws.ge2, SO_XE / 2}, w.xe3, {}, {ws.ze3, SO_XE}, n, SO_XE, SO_XE / 2, ACT_NONE);
    launch_gelu(s, ws.ze3, SO_XE, ws.h + SO_XCOL, SO_H, n, SO_XE, 0);
    // (d) the head (SconeOcc.py:334-342): GELU behind every layer, the last included
    if (g.row_job)
        hipLaunchKernelGGL(so_bcast_rows_kernel, dim3((unsigned)cdiv(n * SO_G, 256)), dim3(256), 0, s, g.gfeat, g.row_job, (long long)g.J, ws.h,
                           (long long)SO_H, (long long)n);
    else launch_copy2d(s, g.gfeat, 0, ws.h, SO_H, n, SO_G);
    launch_copy2d(s, vhc, SO_VH, ws.h + SO_VCOL, SO_H, n, SO_VH);
    vb_linear(s, {ws.h, SO_H}, w.lin1, {}, {ws.z1, SO_L1}, n, SO_L1, SO_H, ACT_NONE);
    launch_gelu(s, ws.z1, SO_L1, ws.g1, SO_L1, n, SO_L1, 0);
    vb_linear(s, {ws.g1, SO_L1}, w.lin2, {}, {ws.z2, SO_L2}, n, SO_L2, SO_L1, ACT_NONE);
    launch_gelu(s, ws.z2, SO_L2, ws.g2, SO_L2, n, SO_L2, 0);
    vb_linear(s, {ws.g2, SO_L2}, w.lin3, {}, {ws.z3, 1}, n, 1, SO_L2, ACT_NONE);
    // (e) the head, backwards
    launch_copy2d(s, d_out_c, 1, ws.dz3, 1, n, 1);
    launch_gelu(s, ws.z3, 1, ws.dz3, 1, n, 1, 1);                                                   // linear3
    gemm_dw(s, ws.dz3, 1, ws.g2, SO_L2, n, 1, SO_L2, DW(OCC_LIN + 2 * LIN_NW + LIN_W), DW(OCC_LIN + 2 * LIN_NW + LIN_B), part);
    gemm_dx(s, ws.dz3, 1, w.lin3.w, SO_L2, ws.d2, SO_L2, n, 1, SO_L2, false, wt);
    launch_gelu(s, ws.z2, SO_L2, ws.d2, SO_L2, n, SO_L2, 1);                                        // linear2
    gemm_dw(s, ws.d2, SO_L2, ws.g1, SO_L1, n, SO_L2, SO_L1, DW(OCC_LIN + LIN_NW + LIN_W), DW(OCC_LIN + LIN_NW + LIN_B), part);
    gemm_dx(s, ws.d2, SO_L2, w.lin2.w, SO_L1, ws.d1, SO_L1, n, SO_L2, SO_L1, false, wt);
    launch_gelu(s, ws.z1, SO_L1, ws.d1, SO_L1, n, SO_L1, 1);                                        // linear1
    gemm_dw(s, ws.d1, SO_L1, ws.h, SO_H, n, SO_L1, SO_H, DW(OCC_LIN + LIN_W), DW(OCC_LIN + LIN_B), part);
    gemm_dx(s, ws.d1, SO_L1, w.lin1.w, SO_H, ws.dH, SO_H, n, SO_L1, SO_H, false, wt);
    // (f) what leaves the head's input as it is: the harmonics' columns, the global features' (summed over the chunk's rows -- one
    // cloud: the bias half of a weight-gradient product of depth 0, then chunk by chunk in order; jobs: so_seg_colsum_kernel)
    if (dvhc) launch_copy2d(s, ws.dH + SO_VCOL, SO_H, dvhc, SO_VH, n, SO_VH);
    if (!deep) return;
    if (dw && g.row_job) {
        hipLaunchKernelGGL(so_seg_colsum_kernel, dim3((unsigned)cdiv(g.J * SO_G, 256)), dim3(256), 0, s, (const float*)ws.dH, (long long)SO_H,
                           g.job_rows, (long long)g.J, (long long)g.r0, (long long)n, g.dG);
    } else if (dw) {
        gemm_dw(s, ws.dH, SO_H, nullptr, 0, n, SO_G, 0, nullptr, g.first_of_cloud ? g.dG : g.gtmp, part);
        if (!g.first_of_cloud) {
            PbSlots slot_g{};                              // one row of the global features' gradient
            slot_g.off[1] = SO_G;
            slot_g.dst[0] = g.dG;
            hipLaunchKernelGGL(pb_add_slots_kernel, dim3(2, 1), dim3(256), 0, s, slot_g, (const float*)g.gtmp);
        }
    }
    // (g) the x-embedding, backwards
    float* dxe = ws.dH + SO_XCOL;
    launch_gelu(s, ws.ze3, SO_XE, dxe, SO_H, n, SO_XE, 1);
    gemm_dw(s, dxe, SO_H, ws.ge2, SO_XE / 2, n, SO_XE, SO_XE / 2, DW(OCC_XE + 2 * LIN_NW + LIN_W), DW(OCC_XE + 2 * LIN_NW + LIN_B), part);
    gemm_dx(s, dxe, SO_H, w.xe3.w, SO_XE / 2, ws.d2, SO_XE / 2, n, SO_XE, SO_XE / 2, false, wt);
    launch_gelu(s, ws.ze2, SO_XE / 2, ws.d2, SO_XE / 2, n, SO_XE / 2, 1);
    gemm_dw(s, ws.d2, SO_XE / 2, ws.ge1, SO_XE / 4, n, SO_XE / 2, SO_XE / 4, DW(OCC_XE + LIN_NW + LIN_W), DW(OCC_XE + LIN_NW + LIN_B), part);
    gemm_dx(s, ws.d2, SO_XE / 2, w.xe2.w, SO_XE / 4, ws.d1, SO_XE / 4, n, SO_XE / 2, SO_XE / 4, false, wt);
    launch_gelu(s, ws.ze1, SO_XE / 4, ws.d1, SO_XE / 4, n, SO_XE / 4, 1);
    gemm_dw(s, ws.d1, SO_XE / 4, xc, 3, n, SO_XE / 4, 3, DW(OCC_XE + LIN_W), DW(OCC_XE + LIN_B), part);
    if (dxc) gemm_dx(s, ws.d1, SO_XE / 4, w.xe1.w, 3, dxc, 3, n, SO_XE / 4, 3, false, wt);
    // (h) the local transformers, backwards, from what (b) left in each scale's scratch (no second forward; each encoder's
    // interior is rebuilt from its boundary as ever); the query's share of the offsets
    for (int i = 0; i < 3; ++i) {
        pb_chunk_backward(s, w.local[i], off[i], ws.dH + SO_LOC + i * SO_LF, n, SO_K, SO_LF / 2, dw ? dw + OCC_LOCAL + i * PCT_NW : nullptr,
                          dxc ? ws.d_off : nullptr, ws.local[i], SO_H, /*forward_done=*/true);
        if (dxc) launch_so_dx_sub(s, ws.d_off, dxc, n);
    }
}

constexpr int64_t SO_RAGGED_MAX_J = 16384;                           // jobs of one mcr_scone_occ_backward_ragged call

}  // namespace
}  // namespace mcr

using namespace mcr;

extern "C" {

// ---- building blocks ---------------------------------------------------------------------------------------------------------------
size_t mcr_attention_backward_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim) {
    return measure(carve_attention_backward, S, L, n_heads, v_dim) + VB_BLOCK_WS_SLACK;
}

int mcr_attention_backward(const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                           int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes,
                           void* stream) {
    const char* who = "mcr_attention_backward";
    MCR_REQUIRE(qkv && d_out && d_qkv, "%s: null pointer", who);
    MCR_REQUIRE(n_heads > 0 && qk_dim == 16 * n_heads && v_dim == 64 * n_heads,
                "%s: per-head widths must be 16 (q, k) and 64 (v), got qk_dim %d, v_dim %d for %d heads", who, qk_dim, v_dim, n_heads);
    MCR_REQUIRE(S > 0 && L > 0 && S <= 65535 && L <= (1 << 30), "%s: bad problem size S=%ld L=%ld", who, (long)S, (long)L);
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldq % 4 == 0 && ld_dout >= v_dim && ld_dout % 4 == 0 && ld_dqkv >= 2 * qk_dim + v_dim &&
                    ld_dqkv % 4 == 0,
                "%s: leading dimensions must cover the rows and be multiples of 4", who);
    MCR_REQUIRE(((uintptr_t)qkv | (uintptr_t)d_out | (uintptr_t)d_qkv) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_attention_backward_workspace_bytes(S, L, n_heads, v_dim), "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    Arena a{(char*)workspace, workspace_bytes};
    const AttnBwdScratch ws = carve_attention_backward(a, S, L, n_heads, v_dim);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    launch_attn_fwd(s, qkv, ldq, ws.O, v_dim, ws.lse, S, (int)L, n_heads, lens, ws.part);
    launch_attn_bwd(s, qkv, ldq, ws.O, v_dim, ws.lse, d_out, ld_dout, ws.delta, d_qkv, ld_dqkv, S, (int)L, n_heads, lens, ws.part);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

size_t mcr_linear_backward_workspace_bytes(int64_t M, int N, int K) {
    return measure(carve_linear_backward, M, N, K) + VB_BLOCK_WS_SLACK;
}

int mcr_linear_backward(const float* X, int64_t ldx, const float* W, const float* Z, int64_t ldz, const float* dY, int64_t ldy, int64_t M, int N,
                        int K, int gelu, float* dX, int64_t ld_dx, int accumulate_dx, float* dW, float* db, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* who = "mcr_linear_backward";
    MCR_REQUIRE(dY && (!dX || W) && ((!dW && !db) || X) && (!gelu || Z), "%s: null pointer", who);   // (db rides on the dW product: it reads X too)
    MCR_REQUIRE(M > 0 && N > 0 && K > 0 && M <= (1ll << 31), "%s: bad problem size M=%ld N=%d K=%d", who, (long)M, N, K);
    MCR_REQUIRE(ldy >= N && (!gelu || ldz >= N) && (!dX || ld_dx >= K) && ((!dW && !db) || ldx >= K), "%s: leading dimension too small", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_linear_backward_workspace_bytes(M, N, K), "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    Arena a{(char*)workspace, workspace_bytes};
    const LinBwdScratch ws = carve_linear_backward(a, M, N, K);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    float* dz = ws.dz;
    const float* g = dY;
    int64_t ldg = ldy;
    if (gelu) {
        launch_copy2d(s, dY, ldy, dz, N, M, N);
        launch_gelu(s, Z, ldz, dz, N, M, N, 1);
        g = dz;
        ldg = N;
    }
    if (dX) gemm_dx(s, g, ldg, W, K, dX, ld_dx, M, N, K, accumulate_dx != 0, ws.wt);
    gemm_dw(s, g, ldg, X, ldx, M, N, K, dW, db, ws.part);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

size_t mcr_layernorm_backward_workspace_bytes(int64_t M, int E) { return measure(carve_layernorm_backward, M, E) + VB_BLOCK_WS_SLACK; }

int mcr_layernorm_backward(const float* X, int64_t ldx, const float* gamma, const float* dY, int64_t ldy, int64_t M, int E, float* dX, int64_t ld_dx,
                           int accumulate_dx, float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_layernorm_backward";
    MCR_REQUIRE(X && gamma && dY && dX, "%s: null pointer", who);
    MCR_REQUIRE(E == 64 || E == 128 || E == 256 || E == 512, "%s: E must be 64, 128, 256 or 512 (got %d)", who, E);
    MCR_REQUIRE(M > 0, "%s: empty problem", who);
    MCR_REQUIRE(ldx >= E && ldy >= E && ld_dx >= E, "%s: leading dimension too small", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_layernorm_backward_workspace_bytes(M, E), "%s: workspace too small", who);
    Arena a{(char*)workspace, workspace_bytes};
    float* part = carve_layernorm_backward(a, M, E);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    launch_ln_bwd((hipStream_t)stream, X, ldx, gamma, dY, ldy, dX, ld_dx, accumulate_dx != 0, d_gamma, d_beta, part, M, E);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

int mcr_colmax_backward(const float* X, int64_t ldx, const float* d_bcast, int64_t ldg, float* dX, int64_t ld_dx, int64_t S, int64_t L, int E,
                        const int* lens, void* stream) {
    const char* who = "mcr_colmax_backward";
    MCR_REQUIRE(X && d_bcast && dX, "%s: null pointer", who);
    MCR_REQUIRE(S > 0 && L > 0 && E > 0 && S <= 65535 && L <= (1 << 30), "%s: bad problem size", who);
    MCR_REQUIRE(ldx >= E && ldg >= E && ld_dx >= E, "%s: leading dimension too small", who);
    launch_colmax_bwd((hipStream_t)stream, X, ldx, d_bcast, ldg, dX, ld_dx, S, (int)L, E, lens);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

// ---- SconeVis ------------------------------------------------------------------------------------------------------------------------
size_t mcr_scone_vis_backward_workspace_bytes(int64_t B, int64_t N) { return (B > 0 && N > 0) ? measure(carve_vb, B, N) + VB_WS_SLACK : 0; }

int mcr_scone_vis_backward(const float* pts, const float* view_harmonics, const float* d_out, int64_t B, int64_t N, const float* const* weights,
                           int n_weights, const int* lengths, float* const* d_weights, float* d_pts, float* d_view_harmonics, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_vis_backward";
    MCR_REQUIRE(pts && view_harmonics && d_out && weights, "%s: null pointer", who);
    if (check_table(who, VIS_TABLE, weights, n_weights, VIS_NW)) return 1;                  // (a planes tail is accepted and ignored)
    MCR_REQUIRE(B > 0 && N > 0 && B <= 65535 && N <= (1 << 24), "%s: bad problem size B=%ld N=%ld", who, (long)B, (long)N);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_vis_backward_workspace_bytes(B, N), "%s: workspace too small", who);
    if (d_weights)
        for (int i = 0; i < VIS_NW; ++i) MCR_REQUIRE(d_weights[i], "%s: d_weights[%d] is null", who, i);
    MCR_REQUIRE(((uintptr_t)pts | (uintptr_t)view_harmonics | (uintptr_t)d_out) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    if (!d_weights && !d_pts && !d_view_harmonics) return 0;
    hipStream_t s = (hipStream_t)stream;
    const VisW w = read_vis_table(weights, VIS_NW);
    const int iN = (int)N;
    const int64_t T = B * N;
    Arena a{(char*)workspace, workspace_bytes};
    const VbScratch ws = carve_vb(a, B, N);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    float* const* X = ws.X;
    float *z1 = ws.z1, *g1 = ws.g1, *hn = ws.hn, *zf1 = ws.zf1, *c2 = ws.c2, *zf2 = ws.zf2, *gf2 = ws.gf2;
    const VbInterior& I = ws.I;
    float *dX = ws.dX, *dH = ws.dH, *dA = ws.dA, *dQKV = ws.dQKV, *delta = ws.delta, *part = ws.part, *wt = ws.wt;
    // where the gradient of the table's entry `slot` goes (d_weights has the table's order and slot names: net_layout.h)
    auto DW = [&](int slot) { return d_weights ? d_weights[slot] : nullptr; };

    // ---- forward of the fp32 network: boundaries X0..X3, the embedding's and the head's pre-activations
    vb_linear(s, {pts, 4}, w.l1, {}, {z1, VB_F}, T, VB_F, 4, ACT_NONE);
    launch_gelu(s, z1, VB_F, g1, VB_F, T, VB_F, 0);
    vb_linear(s, {g1, VB_F}, w.l2, {}, {X[0], VB_E}, T, VB_F, VB_F, ACT_NONE);
    launch_colmax_broadcast(s, X[0], VB_E, X[0] + VB_F, VB_E, B, iN, VB_F, lengths, pts, 4, 4, X[0] + 2 * VB_F);
    for (int e = 0; e < 3; ++e) vb_encoder_fwd(s, w.enc[e], X[e], X[e + 1], I, B, iN, lengths);
    launch_layernorm(s, X[3], VB_E, w.ng, w.nb, hn, VB_E, T, VB_E);
    vb_linear(s, {hn, VB_E}, w.fc1, {}, {zf1, 192}, T, 192, VB_E, ACT_NONE);
    launch_gelu(s, zf1, 192, c2, VB_E, T, 192, 0);
    launch_copy2d(s, view_harmonics, 64, c2 + 192, VB_E, T, 64);
    vb_linear(s, {c2, VB_E}, w.fc2, {}, {zf2, 128}, T, 128, VB_E, ACT_NONE);
    launch_gelu(s, zf2, 128, gf2, 128, T, 128, 0);

    // ---- head (SconeVis.py:143-152), backwards
    gemm_dw(s, d_out, 64, gf2, 128, T, 64, 128, DW(VIS_FC3 + LIN_W), DW(VIS_FC3 + LIN_B), part);                 // fc3
    gemm_dx(s, d_out, 64, w.fc3.w, 128, dH, 128, T, 64, 128, false, wt);
    launch_gelu(s, zf2, 128, dH, 128, T, 128, 1);                                          // fc2
    gemm_dw(s, dH, 128, c2, VB_E, T, 128, VB_E, DW(VIS_FC2 + LIN_W), DW(VIS_FC2 + LIN_B), part);
    gemm_dx(s, dH, 128, w.fc2.w, VB_E, dA, VB_E, T, 128, VB_E, false, wt);
    if (d_view_harmonics) launch_copy2d(s, dA + 192, VB_E, d_view_harmonics, 64, T, 64);
    if (!d_weights && !d_pts) { MCR_LAUNCH_CHECK(who); return 0; }
    launch_gelu(s, zf1, 192, dA, VB_E, T, 192, 1);                                         // fc1
    gemm_dw(s, dA, VB_E, hn, VB_E, T, 192, VB_E, DW(VIS_FC1 + LIN_W), DW(VIS_FC1 + LIN_B), part);
    gemm_dx(s, dA, VB_E, w.fc1.w, VB_E, dH, VB_E, T, 192, VB_E, false, wt);
    launch_ln_bwd(s, X[3], VB_E, w.ng, dH, VB_E, dX, VB_E, false, DW(VIS_NG), DW(VIS_NB), part, T, VB_E);   // norm

    // ---- encoders (Attention.py:278-300), last to first; dX holds the gradient of the encoder's output
    const VbGrads G{dX, dH, dA, dQKV, delta, part, wt};
    for (int e = 2; e >= 0; --e) {
        const int o = VIS_ENC + ENC_NW * e;                               // the encoder's block of the table
        vb_encoder_fwd(s, w.enc[e], X[e], nullptr, I, B, iN, lengths);                    // the interior, from the boundary
        vb_encoder_bwd(s, w.enc[e], d_weights ? d_weights + o : nullptr, X[e], I, G, B, iN, lengths);
    }

    // ---- embedding (Attention.py:98-128): [res | cloud max of res | pts]
    launch_colmax_bwd(s, X[0], VB_E, dX + VB_F, VB_E, dX, VB_E, B, iN, VB_F, lengths);
    gemm_dw(s, dX, VB_E, g1, VB_F, T, VB_F, VB_F, DW(VIS_L2 + LIN_W), DW(VIS_L2 + LIN_B), part);                     // linear2
    gemm_dx(s, dX, VB_E, w.l2.w, VB_F, dH, VB_F, T, VB_F, VB_F, false, wt);
    launch_gelu(s, z1, VB_F, dH, VB_F, T, VB_F, 1);                                        // linear1
    gemm_dw(s, dH, VB_F, pts, 4, T, VB_F, 4, DW(VIS_L1 + LIN_W), DW(VIS_L1 + LIN_B), part);
    if (d_pts) {
        launch_copy2d(s, dX + 2 * VB_F, VB_E, d_pts, 4, T, 4);
        gemm_dx(s, dH, VB_F, w.l1.w, 4, d_pts, 4, T, VB_F, 4, true, wt);
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

// ---- PCTransformer ---------------------------------------------------------------------------------------------------------------------
size_t mcr_attention_backward_pct_workspace_bytes(int64_t S, int64_t L) {
    return measure(carve_attention_backward_pct, S, L) + VB_BLOCK_WS_SLACK;
}

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
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldq % 4 == 0 && ld_dout >= v_dim && ld_dout % 4 == 0 && ld_dqkv >= 2 * qk_dim + v_dim &&
                    ld_dqkv % 4 == 0,
                "%s: leading dimensions must cover the rows and be multiples of 4", who);
    MCR_REQUIRE(((uintptr_t)qkv | (uintptr_t)d_out | (uintptr_t)d_qkv) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (L == 16) {
        launch_attn16_bwd(s, qkv, ldq, d_out, ld_dout, d_qkv, ld_dqkv, S);
        MCR_LAUNCH_CHECK(who);
        return 0;
    }
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_attention_backward_pct_workspace_bytes(S, L), "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    Arena a{(char*)workspace, workspace_bytes};
    const AttnBwdScratch ws = carve_attention_backward_pct(a, S, L);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    launch_attn_fwd(s, qkv, ldq, ws.O, v_dim, ws.lse, S, (int)L, n_heads, lens, ws.part, 8);
    launch_attn_bwd(s, qkv, ldq, ws.O, v_dim, ws.lse, d_out, ld_dout, ws.delta, d_qkv, ld_dqkv, S, (int)L, n_heads, lens, ws.part, 8);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

int mcr_pool_max_avg_backward(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S, int64_t L, int E,
                              void* stream) {
    const char* who = "mcr_pool_max_avg_backward";
    MCR_REQUIRE(X && dY && dX, "%s: null pointer", who);
    MCR_REQUIRE(S > 0 && L > 0 && E > 0 && S <= (1ll << 31) - 1 && L <= (1 << 30) && E <= 64 * 65535, "%s: bad problem size", who);
    MCR_REQUIRE(ldx >= E && ldy >= 2 * E && ld_dx >= E, "%s: leading dimension too small", who);
    launch_pool_bwd((hipStream_t)stream, X, ldx, dY, ldy, dX, ld_dx, S, (int)L, E);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

int mcr_pool_max_avg_backward_lens(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S, int64_t L,
                                   int E, const int* lens, void* stream) {
    const char* who = "mcr_pool_max_avg_backward_lens";
    MCR_REQUIRE(X && dY && dX && lens, "%s: null pointer", who);
    MCR_REQUIRE(S > 0 && L > 0 && E > 0 && S <= (1ll << 31) - 1 && L <= (1 << 30) && E <= 64 * 65535, "%s: bad problem size", who);
    MCR_REQUIRE(ldx >= E && ldy >= 2 * E && ld_dx >= E, "%s: leading dimension too small", who);
    launch_pool_bwd((hipStream_t)stream, X, ldx, dY, ldy, dX, ld_dx, S, (int)L, E, lens);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

int mcr_pc_transformer_backward_chunk(int64_t S, int64_t L) { return (S > 0 && L > 0) ? (int)std::min<int64_t>(pb_chunk(S, L), INT32_MAX) : 0; }

size_t mcr_pc_transformer_backward_workspace_bytes(int64_t S, int64_t L) {
    return (S > 0 && L > 0) ? measure(carve_pb, S, L, 256) + VB_WS_SLACK : 0;          // (sized for the wider feature_dim, 512)
}

int mcr_pc_transformer_backward(const float* pc, const float* d_features, int64_t S, int64_t L, int feature_dim, const float* const* weights,
                                int n_weights, float* const* d_weights, float* d_pc, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_pc_transformer_backward";
    MCR_REQUIRE(pc && d_features && weights, "%s: null pointer", who);
    if (check_table(who, PCT_TABLE, weights, n_weights, PCT_NW)) return 1;                  // (the planes tails are accepted and ignored)
    MCR_REQUIRE(feature_dim == 256 || feature_dim == 512, "%s: feature_dim must be 256 or 512", who);
    MCR_REQUIRE(S > 0 && L > 0 && (L == 16 || S <= 65535) && L <= (1 << 24) && S <= (1ll << 31) / L,
                "%s: bad problem size S=%ld L=%ld (S <= 65535 unless L == 16)", who, (long)S, (long)L);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_pc_transformer_backward_workspace_bytes(S, L), "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    if (d_weights)
        for (int i = 0; i < PCT_NW; ++i) MCR_REQUIRE(d_weights[i], "%s: d_weights[%d] is null", who, i);
    MCR_REQUIRE(((uintptr_t)pc | (uintptr_t)d_features) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    if (!d_weights && !d_pc) return 0;
    hipStream_t s = (hipStream_t)stream;
    const PctW w = read_pct(weights);
    const int half = feature_dim / 2;
    Arena a{(char*)workspace, workspace_bytes};
    const PbScratch ws = carve_pb(a, S, L, half);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const int64_t Sc = pb_chunk(S, L);
    // the chunks behind the first leave their weight gradients in ws.stage, cut in table order, and are added in chunk order
    PbSlots slots{};
    float* stage_tab[PCT_NW];
    if (d_weights && Sc < S)
        for (int i = 0; i < PCT_NW; ++i) {
            slots.dst[i] = d_weights[i];
            slots.off[i + 1] = slots.off[i] + pb_slot_floats(i, half);
            stage_tab[i] = ws.stage + slots.off[i];
        }
    for (int64_t s0 = 0; s0 < S; s0 += Sc) {
        const int64_t n = std::min(Sc, S - s0);
        float* const* dw = !d_weights ? nullptr : s0 == 0 ? d_weights : stage_tab;
        pb_chunk_backward(s, w, pc + s0 * L * 3, d_features + s0 * feature_dim, n, (int)L, half, dw, d_pc ? d_pc + s0 * L * 3 : nullptr, ws);
        if (d_weights && s0 > 0)
            hipLaunchKernelGGL(pb_add_slots_kernel, dim3(64, PCT_NW), dim3(256), 0, s, slots, (const float*)ws.stage);
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

// ---- SconeOcc ------------------------------------------------------------------------------------------------------------------------
int mcr_scone_occ_backward_chunk(int64_t Q) { return Q > 0 ? (int)so_chunk(Q, 0) : 0; }

size_t mcr_scone_occ_backward_workspace_bytes(int64_t B, int64_t Q, int64_t Lg, int64_t q_chunk) {
    return (B > 0 && Q > 0 && Lg > 0 && q_chunk >= 0) ? measure(carve_so, B, so_chunk(Q, q_chunk), Lg) + VB_WS_SLACK : 0;
}

int mcr_scone_occ_backward(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale, const float* x,
                           const float* view_harmonics, const int64_t* const* knn_idx, const float* d_out, int64_t B, int64_t Q,
                           const float* const* weights, int n_weights, float* const* d_weights, float* d_x, float* d_view_harmonics,
                           int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_occ_backward";
    MCR_REQUIRE(pc_global && pc_scale && M_scale && x && view_harmonics && knn_idx && d_out && weights, "%s: null pointer", who);
    if (check_table(who, OCC_TABLE, weights, n_weights, OCC_NW)) return 1;                  // (the planes tails are accepted and ignored)
    MCR_REQUIRE(B > 0 && Q > 0 && Lg > 0 && B <= 65535 && Q <= (1ll << 24) && Lg <= (1 << 24) && B <= (1ll << 31) / Lg &&
                    (Lg != SO_K || B <= PB_CHUNK16),
                "%s: bad problem size B=%ld Q=%ld Lg=%ld", who, (long)B, (long)Q, (long)Lg);
    for (int i = 0; i < 3; ++i) {
        MCR_REQUIRE(pc_scale[i] && knn_idx[i], "%s: scale %d: null pointer", who, i);
        MCR_REQUIRE(M_scale[i] >= SO_K, "%s: scale %d has %ld points (< k = 16)", who, i, (long)M_scale[i]);
        MCR_REQUIRE(((uintptr_t)pc_scale[i] | (uintptr_t)knn_idx[i]) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    }
    MCR_REQUIRE(q_chunk == 0 || (q_chunk >= 16 && q_chunk % 16 == 0 && q_chunk <= (1 << 20)),
                "%s: q_chunk must be 0 (the default) or a multiple of 16 in [16, 2^20], got %ld", who, (long)q_chunk);
    MCR_REQUIRE(((uintptr_t)pc_global | (uintptr_t)x | (uintptr_t)view_harmonics | (uintptr_t)d_out | (uintptr_t)d_x |
                 (uintptr_t)d_view_harmonics) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_occ_backward_workspace_bytes(B, Q, Lg, q_chunk), "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    if (d_weights)
        for (int i = 0; i < OCC_NW; ++i) MCR_REQUIRE(d_weights[i], "%s: d_weights[%d] is null", who, i);
    if (!d_weights && !d_x && !d_view_harmonics) return 0;
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, OCC_NW);
    const int64_t Qc = so_chunk(Q, q_chunk);
    Arena a{(char*)workspace, workspace_bytes};
    const SoScratch ws = carve_so(a, B, Qc, Lg);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const bool deep = d_weights || d_x;                    // anything below the head's input wanted
    SoStage st;
    if (d_weights) so_stage_init(st, d_weights, ws.stage);

    // ---- 1. the global transformer's forward: [B, 512]
    pb_chunk_forward(s, w.global, pc_global, B, (int)Lg, SO_G / 2, ws.global);
    launch_pool_max_avg(s, ws.global.y0, SO_G / 2, ws.gfeat, SO_G, B, (int)Lg, SO_G / 2);

    // ---- 2. cloud by cloud, chunk by chunk
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q0 = 0; q0 < Q; q0 += Qc) {
            const int64_t n = std::min(Qc, Q - q0), r0 = b * Q + q0;
            const bool first = b == 0 && q0 == 0;
            // (a) the neighbourhoods as offsets
            for (int i = 0; i < 3; ++i)
                launch_so_gather(s, pc_scale[i] + b * M_scale[i] * 3, M_scale[i], knn_idx[i] + r0 * SO_K, x + r0 * 3, ws.off[i], n);
            so_chunk_fwd_bwd(s, w, ws, ws.off, x + r0 * 3, view_harmonics + r0 * SO_VH, d_out + r0, n,
                             !d_weights ? nullptr : first ? d_weights : st.tab, d_x ? d_x + r0 * 3 : nullptr,
                             d_view_harmonics ? d_view_harmonics + r0 * SO_VH : nullptr, deep,
                             SoGlobalRows{ws.gfeat + b * SO_G, ws.dG + b * SO_G, ws.gtmp, q0 == 0, nullptr, nullptr, 0, 0});
            if (deep && d_weights && !first) so_stage_add(s, st);
        }

    // ---- 3. the global transformer, backwards (its forward is rebuilt: the chunks have used its scratch)
    if (d_weights) pb_chunk_backward(s, w.global, pc_global, ws.dG, B, (int)Lg, SO_G / 2, d_weights + OCC_GLOBAL, nullptr, ws.global, SO_G);
    MCR_LAUNCH_CHECK(who);
    return 0;
}


// ---- SconeOcc, ragged: J jobs of different sizes, their rows packed into chunks ----------------------------------------------------------
size_t mcr_scone_occ_backward_ragged_workspace_bytes(int64_t J, int64_t T, int64_t Lg, int64_t q_chunk) {
    return (J > 0 && T > 0 && Lg > 0 && q_chunk >= 0) ? measure(carve_so_ragged, J, so_chunk(T, q_chunk), Lg) + VB_WS_SLACK : 0;
}

int mcr_scone_occ_backward_ragged(const float* pc_global, const int* global_len, int64_t Lg, const float* const* offsets, const float* x,
                                  const float* view_harmonics, const int* row_job, const int64_t* job_rows, const float* d_out, int64_t J,
                                  int64_t T, const float* const* weights, int n_weights, float* const* d_weights, float* d_x,
                                  float* d_view_harmonics, int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_occ_backward_ragged";
    MCR_REQUIRE(pc_global && global_len && offsets && x && view_harmonics && row_job && job_rows && d_out && weights, "%s: null pointer", who);
    if (check_table(who, OCC_TABLE, weights, n_weights, OCC_NW)) return 1;                  // (the planes tails are accepted and ignored)
    MCR_REQUIRE(J > 0 && T > 0 && Lg > 0 && J <= SO_RAGGED_MAX_J && T <= (1ll << 24) && Lg <= (1 << 24) && J <= (1ll << 31) / Lg,
                "%s: bad problem size J=%ld T=%ld Lg=%ld (J <= %ld)", who, (long)J, (long)T, (long)Lg, (long)SO_RAGGED_MAX_J);
    MCR_REQUIRE(Lg != SO_K, "%s: global sequences of 16 tokens are not supported (their fused attention backward takes no lens)", who);
    for (int i = 0; i < 3; ++i) {
        MCR_REQUIRE(offsets[i], "%s: scale %d: null pointer", who, i);
        MCR_REQUIRE((uintptr_t)offsets[i] % 16 == 0, "%s: operands must be 16-byte aligned", who);
    }
    MCR_REQUIRE(q_chunk == 0 || (q_chunk >= 16 && q_chunk % 16 == 0 && q_chunk <= (1 << 20)),
                "%s: q_chunk must be 0 (the default) or a multiple of 16 in [16, 2^20], got %ld", who, (long)q_chunk);
    MCR_REQUIRE(((uintptr_t)pc_global | (uintptr_t)x | (uintptr_t)view_harmonics | (uintptr_t)d_out | (uintptr_t)d_x |
                 (uintptr_t)d_view_harmonics) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    MCR_REQUIRE((uintptr_t)global_len % 4 == 0 && (uintptr_t)row_job % 4 == 0 && (uintptr_t)job_rows % 8 == 0,
                "%s: global_len, row_job (4 bytes) and job_rows (8 bytes) must be aligned to their element", who);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_occ_backward_ragged_workspace_bytes(J, T, Lg, q_chunk), "%s: workspace too small", who);
    MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    if (d_weights)
        for (int i = 0; i < OCC_NW; ++i) MCR_REQUIRE(d_weights[i], "%s: d_weights[%d] is null", who, i);
    if (!d_weights && !d_x && !d_view_harmonics) return 0;
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, OCC_NW);
    const int64_t Qc = so_chunk(T, q_chunk);
    Arena a{(char*)workspace, workspace_bytes};
    const SoRaggedScratch rs = carve_so_ragged(a, J, Qc, Lg);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const SoScratch& ws = rs.so;
    const bool deep = d_weights || d_x;
    SoStage st;
    if (d_weights) so_stage_init(st, d_weights, ws.stage);

    // ---- 1. the global transformer's forward over the J padded sequences: [J, 512]; nothing of the caller's padding is read again
    hipLaunchKernelGGL(so_pad_global_kernel, dim3((unsigned)cdiv(J * Lg * 3, 256)), dim3(256), 0, s, pc_global, global_len, rs.pcg, (long long)J,
                       (int)Lg);
    pb_chunk_forward(s, w.global, rs.pcg, J, (int)Lg, SO_G / 2, ws.global, global_len);
    launch_pool_max_avg(s, ws.global.y0, SO_G / 2, ws.gfeat, SO_G, J, (int)Lg, SO_G / 2, global_len);
    if (d_weights)
        if (int e = check_hip(hipMemsetAsync(ws.dG, 0, (size_t)J * SO_G * sizeof(float), s), who)) return e;

    // ---- 2. the rows of all jobs, chunk by chunk
    const float* off[3];
    for (int64_t r0 = 0; r0 < T; r0 += Qc) {
        const int64_t n = std::min(Qc, T - r0);
        for (int i = 0; i < 3; ++i) off[i] = offsets[i] + r0 * SO_K * 3;
        so_chunk_fwd_bwd(s, w, ws, off, x + r0 * 3, view_harmonics + r0 * SO_VH, d_out + r0, n, !d_weights ? nullptr : r0 == 0 ? d_weights : st.tab,
                         d_x ? d_x + r0 * 3 : nullptr, d_view_harmonics ? d_view_harmonics + r0 * SO_VH : nullptr, deep,
                         SoGlobalRows{ws.gfeat, ws.dG, nullptr, false, row_job + r0, (const long long*)job_rows, J, r0});
        if (deep && d_weights && r0 > 0) so_stage_add(s, st);
    }

    // ---- 3. the global transformer, backwards, job by job in job order (its forward is rebuilt: the chunks have used its scratch).  One
    // job's gradient depends on nothing but that job -- a job without rows has dG = 0 and adds exact zeros
    if (d_weights) {
        PbSlots slots{};
        float* stage_tab[PCT_NW];
        for (int i = 0; i < PCT_NW; ++i) {
            slots.dst[i] = d_weights[OCC_GLOBAL + i];
            slots.off[i + 1] = slots.off[i] + pb_slot_floats(i, SO_G / 2);
            stage_tab[i] = rs.global1.stage + slots.off[i];
        }
        for (int64_t j = 0; j < J; ++j) {
            pb_chunk_backward(s, w.global, rs.pcg + j * Lg * 3, ws.dG + j * SO_G, 1, (int)Lg, SO_G / 2, j == 0 ? d_weights + OCC_GLOBAL : stage_tab,
                              nullptr, rs.global1, SO_G, false, global_len + j);
            if (j > 0) hipLaunchKernelGGL(pb_add_slots_kernel, dim3(64, PCT_NW), dim3(256), 0, s, slots, (const float*)rs.global1.stage);
        }
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

}  // extern "C"
