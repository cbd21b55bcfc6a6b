// Building blocks of the networks' backward passes for gfx950 (MI355X) (each behind its own C entry point, include/macarons_hip.h):
//   linear      dZ = dY * GELU'(Z) (exact erf: Phi(z) + z phi(z)); dX = dZ W (written or added) on the forward's exact-fp32 MFMA GEMM
//               through a transposed weight copy; dW | db = dZ^T [X | 1] as a VALU split-K GEMM whose slabs are summed in a fixed order.
//   layernorm   per row mu, sigma recomputed (eps 1e-5); dx added into (or written to) the residual gradient; d_gamma | d_beta as
//               per-block column partials summed in a fixed order.
//   column max  the arg-max valid row of each column (ties: the lowest row, as torch.max(dim)) receives the column's gradient
//               summed over all rows.
// (Numerics and determinism: as stated in scone_vis_bwd.hip, for every entry of the backward sources.)
// The PCTransformer tail's pooling has its own backward (pb_pool_bwd_kernel).  lin_fwd / lin_bwd: the networks' one linear layer.
#include "bwd_kernels.h"

namespace mcr {
namespace {
typedef float f2 __attribute__((ext_vector_type(2)));

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

// the workspaces of the building-block entries
struct LinBwdScratch { float *dz, *part, *wt; };
LinBwdScratch carve_linear_backward(Arena& a, int64_t M, int N, int K) {
    LinBwdScratch w;
    w.dz = a.f((size_t)M * N);
    w.part = a.f(vb_gradw_floats(M, N, K));
    w.wt = a.f((size_t)N * K);
    return w;
}
float* carve_layernorm_backward(Arena& a, int64_t M, int E) { return a.f(vb_ln_part_floats(M, E)); }

// the two pooling entries: lens is required by the one (need_lens) and absent from the other
int pool_max_avg_backward(const char* who, const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S,
                          int64_t L, int E, const int* lens, bool need_lens, void* stream) {
    MCR_REQUIRE(X && dY && dX && (lens || !need_lens), "%s: null pointer", who);
    MCR_REQUIRE(S > 0 && L > 0 && E > 0 && S <= (1ll << 31) - 1 && L <= (1 << 30) && E <= 64 * 65535, "%s: bad problem size", who);
    MCR_REQUIRE(ldx >= E && ldy >= 2 * E && ld_dx >= E, "%s: leading dimension too small", who);
    launch_pool_bwd((hipStream_t)stream, X, ldx, dY, ldy, dX, ld_dx, S, (int)L, E, lens);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

inline int vb_ln_rows(int64_t M) { return (int)std::max<long long>(16, cdiv(cdiv(M, 256), 4) * 4); }
}  // namespace

// ---- the launchers and size functions of bwd_kernels.h -----------------------------------------------------------------------------------
size_t vb_gradw_floats(int64_t M, int N, int K) { return (size_t)vb_slabs(M) * N * (K + 1); }
size_t vb_ln_part_floats(int64_t M, int E) { return (size_t)cdiv(M, vb_ln_rows(M)) * E * 2; }

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
void launch_colmax_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dG, int64_t ldg, float* dX, int64_t ldd, int64_t S, int L,
                       int E, const int* lens) {
    hipLaunchKernelGGL(vb_colmax_bwd_kernel, dim3((unsigned)cdiv(E, 64), (unsigned)S), dim3(1024), 0, s, X, (long long)ldx, dG, (long long)ldg,
                       dX, (long long)ldd, L, E, lens);
}
void launch_pool_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ldd, int64_t S, int L, int E,
                     const int* lens) {
    const dim3 grid((unsigned)S, (unsigned)cdiv(E, 64));
    const long long lx = ldx, ly = ldy, ld = ldd;
    if (lens) hipLaunchKernelGGL(pb_pool_bwd_lens_kernel, grid, dim3(1024), 0, s, X, lx, dY, ly, dX, ld, L, E, lens);
    else hipLaunchKernelGGL(pb_pool_bwd_kernel, grid, dim3(1024), 0, s, X, lx, dY, ly, dX, ld, L, E);
}

void lin_fwd(hipStream_t s, int64_t T, LinShape L, const LinW& w, Rows X, Rows R, RowsOut Y, RowsOut G) {
    launch_linear(s, X, {w.w, L.K}, {w.b, ACT_NONE, R}, Y, T, L.N, L.K, /*route_rows=*/1);
    if (G.p) launch_gelu(s, Y.p, Y.ld, G.p, G.ld, T, L.N, 0);
}

void lin_bwd(const LinCtx& c, LinShape L, const LinW& w, int slot, Rows Z, RowsOut dY, Rows X, RowsOut dX, bool accumulate) {
    if (Z.p) launch_gelu(c.s, Z.p, Z.ld, dY.p, dY.ld, c.T, L.N, 1);
    if (c.dw && slot != LIN_NO_DW) gemm_dw(c.s, dY.p, dY.ld, X.p, X.ld, c.T, L.N, L.K, c.dw[slot + LIN_W], c.dw[slot + LIN_B], c.part);
    if (dX.p) gemm_dx(c.s, dY.p, dY.ld, w.w, L.K, dX.p, dX.ld, c.T, L.N, L.K, accumulate, c.wt);
}
}  // namespace mcr
using namespace mcr;
extern "C" {
size_t mcr_linear_backward_workspace_bytes(int64_t M, int N, int K) { return measure(carve_linear_backward, M, N, K) + VB_BLOCK_WS_SLACK; }

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
    float* const dz = ws.dz;
    const float* g = dY;
    int64_t ldg = ldy;
    if (gelu) {
        launch_copy2d(s, dY, ldy, dz, N, M, N);
        launch_gelu(s, Z, ldz, dz, N, M, N, 1);
        g = dz;
        ldg = N;
    }
    if (dX) gemm_dx(s, g, ldg, W, K, dX, ld_dx, M, N, K, accumulate_dx != 0, ws.wt);     // (dX before dW here: lin_bwd has the networks' order)
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

int mcr_pool_max_avg_backward(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S, int64_t L, int E,
                              void* stream) {
    return pool_max_avg_backward("mcr_pool_max_avg_backward", X, ldx, dY, ldy, dX, ld_dx, S, L, E, nullptr, false, stream);
}

int mcr_pool_max_avg_backward_lens(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S, int64_t L,
                                   int E, const int* lens, void* stream) {
    return pool_max_avg_backward("mcr_pool_max_avg_backward_lens", X, ldx, dY, ldy, dX, ld_dx, S, L, E, lens, true, stream);
}

}  // extern "C"
