// Device-side building blocks of the SCONE networks (K4-K8 of SURVEY §2.3) for gfx950.
// Launch helpers are declared here and defined in nn_kernels.hip; the network files (pct.hip, scone_vis.hip, scone_occ.hip) compose them.
#pragma once
#include "common.h"

namespace mcr {

enum Act { ACT_NONE = 0, ACT_GELU = 1 };

// ---- operands of the launch helpers.  Host side only: every launcher unpacks them into its kernel's own parameter list. ----
// fp32 rows: row m starts at p + m * ld floats.  A null p means "absent" (no residual, no fp32 output).
struct Rows { const float* p; int64_t ld; };
struct RowsOut { float* p; int64_t ld; };
// An fp16 hi/lo plane pair (value = h + l), rows of ld halves.  l == nullptr: the high plane alone (variant 7).
struct Planes {
    _Float16 *h, *l; int64_t ld;
    Planes cols(int64_t c) const { return {h + c, l ? l + c : nullptr, ld}; }           // both planes advanced by c columns
    Planes high() const { return {h, nullptr, ld}; }
    Planes keep(int n_planes) const { return n_planes == 1 ? high() : *this; }          // the planes an n_planes product reads / writes
};
// the back-to-back layout: two [rows][width] fp16 arrays over one scratch region (an fp32 row of the region holds two fp16 rows)
inline Planes planes_over(void* base, int64_t rows, int64_t width) {
    _Float16* h = reinterpret_cast<_Float16*>(base);
    return {h, h + rows * width, width};
}
// Weight planes [2][N][ld] of W * 2^e travel with inv_scale = 2^-e, the inverse of the power of two they were split with.
struct WPlanes { const _Float16 *h, *l; int64_t ld; float inv_scale; };
// an extra bias per group of rows: p[g * N + n], g = row_group[m] (device int per row) when given, else m / rows_per_group
struct RowBias { const float* p; int64_t rows_per_group; const int* row_group; };
// what a GEMM does behind the product: + bias[n] (+ row bias), act, + residual[m * ld + n] (fp32 output only)
struct Epilogue { const float* bias; int act; Rows residual; RowBias row_bias; };

// Y[m, n] = act( sum_k X[m, k] * W[n, k] + bias[n] ) (+ residual[m, n]);   m < M, n < N
// nn.Linear semantics (W is [N,K] row-major, row stride W.ld).  fp32 MFMA (v_mfma_f32_32x32x2_f32), exact-fp32 products.
// e.row_bias (optional) folds the per-cloud global feature of SconeOcc into the head's first layer without materialising the concat.
// route_rows (0 = M): the row count the fp32 / split-precision routing decision is taken on.  The networks pass the rows of ONE
// cloud / sequence, so that a cloud's numerics do not depend on how many other clouds share the launch (a scene batch, a
// query shard of a multi-GPU step and the single-cloud call then agree bit for bit); the tiling (nt) may still follow M: every
// fp32 tiling accumulates k in the same order.
void launch_linear(hipStream_t s, Rows X, Rows W, const Epilogue& e, RowsOut Y, int64_t M, int N, int K, int64_t route_rows);

// Split-precision variant for the large GEMMs (linear3.hip): the operands' split into bf16 hi/mid/lo is exact, the product keeps six
// of the nine plane products -- the three dropped ones stay below 2^-21 sum_k |x||w| (derivation in linear3.hip) -- ; launch_linear
// routes to it when linear3_applicable().
bool linear3_shape_ok(const float* X, int64_t ldx, const float* W, int64_t ldw, int N, int K);
bool linear3_applicable(const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t M, int N, int K);
void launch_linear3(hipStream_t s, Rows X, Rows W, const Epilogue& e, RowsOut Y, int64_t M, int N, int K);

// Two-term fp16 split variant (linear3h.hip, three MFMAs per product) on fp32 rows of X and weight planes [2][N][K] (the host's, or
// launch_split_weights' into linear3h_planes_bytes(N, K) bytes of scratch).  Range |x| < 65504, |w| < 255.
bool linear3h_applicable(const float* X, int64_t ldx, const float* W, int64_t ldw, int64_t M, int N, int K);
size_t linear3h_planes_bytes(int N, int K);
void launch_linear3h(hipStream_t s, Rows X, WPlanes W, const Epilogue& e, RowsOut Y, int64_t M, int N, int K);

// Row LayerNorm (eps 1e-5, affine): Y[m, :E] = (X[m, :E] - mean) * rstd * g + b     (Attention.py:274,292)
void launch_layernorm(hipStream_t s, const float* X, int64_t ldx, const float* g, const float* b, float* Y, int64_t ldy,
                      int64_t M, int E);

// Multi-head self-attention core on a packed QKV buffer (Attention.py:8-36,174-198; mask=None, no dropout):
//   qkv[m, 0:DQK | DQK:2DQK | 2DQK:2DQK+DV], head h owns channels [h*d,(h+1)*d); scores / sqrt(dqk_per_head);
//   out[m, h*dv:(h+1)*dv].   Sequences are S consecutive blocks of L rows.
//   lens (optional, device int per sequence): keys = the first min(L, lens[s]) rows (padded variable-length batches).
// AttnMask (p null: none; bytes; Attention.py:24-27): pair (sequence s, head h, query q, key k) is masked where
//   p[s * ms + h * mh + q * mq + k] == 0: its score becomes -1e3 BEFORE the 1/sqrt(d) scale (so a fully masked query attends
//   uniformly, as upstream); strides of 0 broadcast (a [S, L] key mask: query stride 0).
struct AttnMask { const unsigned char* p; long long ms, mh, mq; };
// AttnSplit (ws null: none; attention_split_floats(S, L, H, DV) floats): lets long sequences (L >= 512) split their keys over two
// blocks.  mode 1: whenever L >= 512, whatever S -- the networks use this so that a cloud's result does not depend on how many clouds
// share the launch (the two forms differ by summation order, ~1e-6); -1: only when the unsplit grid leaves CUs idle (at most 256
// blocks); 0: never.
struct AttnSplit { float* ws; size_t floats; int mode; };
void launch_attention(hipStream_t s, Rows qkv, RowsOut out, int64_t S, int L, int H, int DQK, int DV, const int* lens, AttnSplit split,
                      bool pv_half);
void launch_attention(hipStream_t s, Rows qkv, RowsOut out, int64_t S, int L, int H, int DQK, int DV, const int* lens, AttnSplit split,
                      const AttnMask& mask);
// planes: when the key-split form runs, its combine pass writes the result as fp16 hi/lo planes INSTEAD of fp32 rows of `out`; the
// return value says whether that happened (else `out` holds fp32 rows as usual)
bool launch_attention(hipStream_t s, Rows qkv, RowsOut out, int64_t S, int L, int H, int DQK, int DV, const int* lens, AttnSplit split,
                      bool pv_half, Planes planes);
size_t attention_split_floats(int64_t S, int L, int H, int DV);
// the merge pass of the key-split form: out <- (w0 out + w1 part1) / (w0 l0 + w1 l1) per (row, head), as planes P when P.h is set,
// else as fp32 rows of out
void launch_attention_combine(hipStream_t s, RowsOut out, const float* part1, const float* ml, int64_t T, int H, int dv, Planes P);
// The same attention on a packed q | k | v operand that already is a pair of fp16 hi/lo planes (attention_planes.hip): K / V tiles by
// LDS DMA, nothing split inside.  Result: planes O when O.h is set, else fp32 rows of out (out is also the scratch of the key-split
// form's first part).  n_planes = 1: the high planes alone (variant 7; P.l / O.l unused, never split)
bool attention_planes_applicable(int H, int DQK, int DV, int64_t ldp);
void launch_attention_planes(hipStream_t s, Planes P, RowsOut out, Planes O, int64_t S, int L, int H, int DQK, int DV, const int* lens,
                             AttnSplit split, int n_planes);

// Column max over the L rows of each of S sequences, broadcast into a column slice of every row:
//   Y[(s*L + r)*ldy + c] = max_r' X[(s*L + r')*ldx + c], c < E          (Embedding global feature, Attention.py:117-121)
// `ex` (optional): ex_cols columns of a second [S*L, ex_ld] array copied to ex_dst (leading dimension ldy) on the way -- inside the
// same launch for the long sequences (L >= 512, ex_cols <= 16), by a copy launch otherwise.
void launch_colmax_broadcast(hipStream_t s, const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int L, int E,
                             const int* lens = nullptr, const float* ex = nullptr, int ex_ld = 0, int ex_cols = 0, float* ex_dst = nullptr);

// PCTransformer tail (SconeOcc.py:123-126): per sequence, max over rows then mean over rows:
//   Y[s*ldy + c] = max_r X[(s*L+r)*ldx + c],  Y[s*ldy + E + c] = mean_r X[...]
void launch_pool_max_avg(hipStream_t s, const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int L, int E,
                         const int* lens = nullptr);   // lens: rows of sequence s that take part (padded batches)

// Strided 2-D copy: Y[m*ldy + c] = X[m*ldx + c], c < E
void launch_copy2d(hipStream_t s, const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t M, int E);

// Fused per-query local PCTransformer (local_pct.hip): offs [S,16,3] -> feat[s*ld_feat + 0:256] (max || avg).
// `blob` is the host-packed parameter image of one local transformer (local_pct_blob_floats() floats).
void launch_local_pct(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob);
void launch_local_pct5(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob);   // bf16 hi/mid/lo blob
// fp16 hi/lo blob; feat_h / feat_l (optional): write the features as fp16 hi/lo planes (row stride ld_feat halves) instead of fp32
void launch_local_pct6(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob,
                       void* feat_h = nullptr, void* feat_l = nullptr);
// variant 7 (opt-in 16-bit matrix path): ONE fp16 plane per operand (local_pct7.hip); feat_h (optional): the features as one fp16 plane
void launch_local_pct7(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob, void* feat_h = nullptr);

// Head GEMM on operands that already are fp16 hi/lo planes in HBM (linear3p.hip): Y (fp32 rows, or planes) = act(X W^T 2^-e + bias ...)
// n_planes = 1: the high planes alone, one MFMA per product (variant 7); X.l / W.l / Y.l unused
bool linear3p_applicable(int N, int K, int64_t ldx, int64_t ldw, int64_t ldy);
void launch_linear3p(hipStream_t s, Planes X, WPlanes W, const Epilogue& e, RowsOut Y, int64_t M, int N, int K, int n_planes);
void launch_linear3p(hipStream_t s, Planes X, WPlanes W, const Epilogue& e, Planes Y, int64_t M, int N, int K, int n_planes);   // (no residual)
// LayerNorm whose output leaves as fp16 hi/lo planes: the input of a planes GEMM, split where it is produced (Y.l null: high plane alone)
void launch_layernorm_planes(hipStream_t s, Rows X, const float* g, const float* b, Planes Y, int64_t M, int E);
// act(X W^T + bias) for K <= 4 (W dense [N, K]) as planes, always both.  Np > N: columns N .. Np - 1 are written as zeros -- a padded K
// for the consuming GEMM
void launch_linear_smallk_planes(hipStream_t s, Rows X, const float* W, const float* bias, int act, Planes Y, int64_t M, int N, int K, int Np);
// out[m] = act2( act(X W^T 2^-e + e.bias)[m][:] . v + c ) for a 256-feature layer: two layers, one launch
void launch_linear3p_dot(hipStream_t s, Planes X, WPlanes W, const Epilogue& e, int64_t M, int K, const float* v, const float* c, int act2,
                         float* out, int n_planes);
void launch_split_to_planes(hipStream_t s, Rows X, Planes P, int64_t M, int E);      // (P.l null: high plane alone)
constexpr float WSPLIT_INV = 1.0f / 256.0f;   // WPlanes::inv_scale of what the two launchers below write
void launch_split_weights(hipStream_t s, const float* W, int64_t ldw, void* planes, int N, int K);   // linear3h.hip: [2][N][K] fp16 of W * 2^8
// the same with zero padding to [2][Np][Kp] (Np % 4 == 0, Kp % 32 == 0) and the bias padded to bias_p [Np]
void launch_pad_weights(hipStream_t s, const float* W, int64_t ldw, const float* bias, void* planes, float* bias_p, int N, int K, int Np, int Kp);
// segmented kNN-16 with query offsets (knn.hip): see launch_knn16_segmented there
void launch_knn16_segmented(hipStream_t s, const float* X, const float* pc, const long long* pc_off, const int* blocks,
                            int64_t n_blocks, int64_t T, float* offsets_out, float* split_ws = nullptr, int slice = 0);
size_t knn16_segmented_split_floats(int64_t T);
int knn_rows_per_block();
// grid-pruned exact kNN-16 (knn.hip: K1-grid): query order once per query set, one sorted copy per candidate cloud
struct KnnGridCloud { const void* cand; const void* boxes; const void* hdr; int64_t cand_stride, box_stride; };
bool knn_grid_applicable(int64_t M, int k);
size_t knn_grid_query_bytes(int64_t B, int64_t Q);
size_t knn_grid_cloud_bytes(int64_t B, int64_t M);
size_t knn_grid_park_bytes();
const int* knn_grid_order_queries(hipStream_t s, const float* X, int64_t B, int64_t Q, void* ws, void* park_ws, bool launch = true);
KnnGridCloud knn_grid_build_cloud(hipStream_t s, const float* pc, int64_t B, int64_t M, void* ws);
void knn_grid_build_clouds(hipStream_t s, int n, const float* const* pc, const int64_t* M, int64_t B, void* const* ws, KnnGridCloud* out);
void launch_knn16_grid(hipStream_t s, const float* X, const float* pc, int64_t M, const int* qperm, const KnnGridCloud& c, int64_t b_first,
                       int64_t n_b, int64_t Q, int64_t* idx, float* dist, float* pts, bool offsets, void* park_ws, int launch);
int local_pct_blob_floats();
int local_pct5_blob_floats();
int local_pct6_blob_floats();
int local_pct7_blob_floats();

}  // namespace mcr
