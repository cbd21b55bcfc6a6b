/* macarons_hip.h — C ABI of libmacarons_hip.so: the MI355X (gfx950) kernels of the SCONE
 * coverage-gain hot path of MACARONS.
 *
 * The reference (Anttwo/MACARONS) is pure Python/PyTorch: it has no FFI.  Its boundary for this path
 * is the Python class surface of macarons/networks/{SconeVis,SconeOcc,Macarons}.py, which
 * macarons_amd/networks mirrors.  THIS header is the layer below it: plain pointers and sizes, no
 * torch types.  Every entry point cites the reference op sequence (file:line, relative to the
 * upstream tree) it replaces.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP, gfx950) to contiguous row-major fp32 unless stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return 0 on success; non-zero on error, message via mcr_last_error() (thread-local): 1 = an argument check of the entry point,
 *     2 = a HIP error, 3 = a kernel launcher refused (part of) the call after the entry's own checks -- nothing was launched for it;
 *   - no entry point allocates device memory: scratch is passed in (`*_workspace_bytes` gives size).
 */
#ifndef MACARONS_HIP_H
#define MACARONS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* mcr_last_error(void);
int mcr_abi_version(void);
const char* mcr_target_arch(void);

/* ---- K9: SH coverage-gain scorer -----------------------------------------------------------------
 * Replaces SconeVis.compute_coverage_gain (macarons/networks/SconeVis.py:210-252):
 *   gains[b,c] = mean_n act( sum_k Y_k(dir(cams[b,c] - pts[b,n,:3])) * harmonics[b,n,k] )
 * with the real SH basis of macarons/utility/spherical_harmonics.py:111-157 in the angle convention
 * of macarons/utility/CustomGeometry.py:27-45; act = sigmoid (use_sigmoid) or relu (SconeVis.py:242-245).
 *   pts [B,N,pts_dim] (pts_dim >= 3, only xyz read — SconeVis.py:224), harmonics [B,N,64],
 *   cams [B,C,3], gains [B,C].  waves_per_simd: grid sizing override, 0 = auto (whole grid co-resident).
 * Deterministic (two-pass reduce, no float atomics). */
size_t mcr_sh_coverage_gain_workspace_bytes(int64_t B, int64_t N, int64_t C);
int mcr_sh_coverage_gain(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* gains,
                         int64_t B, int64_t N, int64_t C, int use_sigmoid, int waves_per_simd, void* workspace,
                         size_t workspace_bytes, void* stream);
/* First stage of mcr_sh_coverage_gain alone (sh_gain_kernel: per-(wave tile, camera) partial sums left in `workspace`), so that
 * the dominant kernel can be timed by itself (bench.py roofline); same arguments minus `gains`. */
int mcr_sh_coverage_gain_partials(const float* pts, int pts_dim, const float* harmonics, const float* cams, int64_t B, int64_t N,
                                  int64_t C, int use_sigmoid, int waves_per_simd, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* mcr_sh_coverage_gain + the decision behind it (testers/shapenet.py:172: torch.max over the cameras) in one call: record [B,2] =
 * (max_c gains[b,c], first arg-max camera as fp32; a NaN gain wins like torch.max; C < 2^24). */
int mcr_sh_coverage_gain_best(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* gains, float* record,
                              int64_t B, int64_t N, int64_t C, int use_sigmoid, int waves_per_simd, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Replaces SconeVis.compute_visibilities (SconeVis.py:164-208) == Macarons.compute_visibility_gains
 * (macarons/networks/Macarons.py:138-178): the same without the mean.  vis [B,C,N]. */
int mcr_sh_visibilities(const float* pts, int pts_dim, const float* harmonics, const float* cams, float* vis,
                        int64_t B, int64_t N, int64_t C, int use_sigmoid, void* stream);

/* ---- K9 backward: gradients of the scorer ---------------------------------------------------------
 * The backward of out = act(z),  z[b,c,n] = sum_k Y_k(dir(cams[b,c] - pts[b,n,:3])) * harmonics[b,n,k]  (the function of
 * mcr_sh_coverage_gain / mcr_sh_visibilities).  grad is the upstream gradient: gains [B,C] (grad_per_pair = 0; the per-pair weight is
 * grad[b,c] / N) or per-pair [B,C,N] (grad_per_pair != 0).  With s = act'(z) * weight (sigmoid: sigma (1 - sigma); relu: 1 where z > 0,
 * 0 elsewhere, as torch's threshold_backward) and u = grad_d z, the gradient of z along the ray d = cams[b,c] - pts[b,n,:3]:
 *   d_harm [B,N,64]      = sum_c s * Y(dir)
 *   d_pts  [B,N,pts_dim] = -sum_c s * u   (channels >= 3 are 0)
 *   d_cams [B,C,3]       = sum_n s * u
 * An output pointer may be NULL: that gradient is neither computed nor written (d_harm alone skips the direction derivatives).
 * workspace: mcr_sh_scorer_backward_workspace_bytes(B, N, C) bytes of device scratch.  Deterministic (fixed-order partial sums,
 * no float atomics): two calls on the same inputs give bit-identical gradients. */
size_t mcr_sh_scorer_backward_workspace_bytes(int64_t B, int64_t N, int64_t C);
int mcr_sh_scorer_backward(const float* pts, int pts_dim, const float* harmonics, const float* cams, const float* grad, int grad_per_pair,
                           int use_sigmoid, float* d_harm, float* d_pts, float* d_cams, int64_t B, int64_t N, int64_t C, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- K1: k nearest surface points per query ---------------------------------------------------------
 * Replaces get_knn_points (macarons/utility/utils.py:1497-1509: torch.cdist + topk(largest=False) +
 * pytorch3d.ops.knn_gather) and, with subtract_query != 0, the offset step of SconeOcc.forward
 * (macarons/networks/SconeOcc.py:297-298).
 *   X [B,Q,3] queries, pc [B,M,3] surface points ->
 *   idx [B,Q,k] int64 (ascending distance; ties -> lower index), dists [B,Q,k], pts [B,Q,k,3]
 *   (neighbour coordinates, minus the query if subtract_query).  k in {1,4,8,16}, k <= M.  idx and / or dists may be NULL
 *   (not written: SconeOcc only consumes the offsets). */
int mcr_knn_points(const float* X, const float* pc, int64_t* idx, float* dists, float* pts, int64_t B, int64_t Q,
                   int64_t M, int k, int subtract_query, void* stream);

/* The same search with a scratch buffer (mcr_knn_grid_workspace_bytes(B, Q, M) bytes, device): for k = 16 and 1024 <= M <= 16384 the
 * candidates are counting-sorted into a 16^3 Morton grid, the queries into a 32^3 one, and a wave visits only the 32-candidate
 * sub-tiles whose bounding box can still hold one of its queries' 16 nearest points -- outputs IDENTICAL to mcr_knn_points (same
 * exact fp32 distances, same (distance, index) order); any other shape runs mcr_knn_points itself.  Nothing upstream corresponds to
 * the pruning: torch.cdist + topk (utils.py:1497-1509) is brute force. */
size_t mcr_knn_grid_workspace_bytes(int64_t B, int64_t Q, int64_t M);
int mcr_knn_points_grid(const float* X, const float* pc, int64_t* idx, float* dists, float* pts, int64_t B, int64_t Q, int64_t M,
                        int k, int subtract_query, void* workspace, size_t workspace_bytes, void* stream);

/* The k = 16 search of J independent jobs in one launch (the ragged occupancy pass, macarons_utils.py:1395-1540: every (cell, chunk)
 * job runs utils.py:1497-1509 + SconeOcc.py:297-298 on its own cloud): X [T,3] query rows sorted by job; pc = the jobs' clouds
 * back to back, job j = rows pc_off[j] .. pc_off[j+1] (device int64 [J+1], every job >= 16 points); blocks (device int32
 * [n_blocks,4]) = (job, first query row, rows <= mcr_knn_rows_per_block(), 0), one workgroup each; offsets_out [T,16,3] = neighbour
 * minus query, neighbours in mcr_knn_points' order.  workspace (optional, mcr_knn_offsets_segmented_workspace_bytes(T) bytes): lets a
 * launch with few blocks split every job's candidates over several workgroups (same result). */
size_t mcr_knn_offsets_segmented_workspace_bytes(int64_t T);
int mcr_knn_offsets_segmented(const float* X, const float* pc, const int64_t* pc_off, const int* blocks, int64_t n_blocks, int64_t T,
                              float* offsets_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K4/K5 building blocks (macarons/networks/Attention.py) -------------------------------------------
 * mcr_linear: nn.Linear (+ optional exact-erf GELU, + optional residual add):
 *   Y[m*ldy+n] = act(sum_k X[m*ldx+k] * W[n*K+k] + bias[n]) + residual[m*ldr+n]     (Attention.py:98-103,186-188,232-235)
 * mcr_layernorm: nn.LayerNorm(E), eps 1e-5 (Attention.py:274,292).
 * mcr_attention: attention() of Attention.py:8-36 with the head split of :174-198 on a packed row
 *   [q (qk_dim) | k (qk_dim) | v (v_dim)], head h owning channels [h*d,(h+1)*d); mask = None; S sequences of
 *   L consecutive rows; scores are divided by sqrt(qk_dim / n_heads).  Supported: 4 heads, (32,128) | (64,256).
 * mcr_colmax_broadcast: Embedding's cloud-wide max feature (Attention.py:117-121).
 * mcr_pool_max_avg: PCTransformer's max || avg pooling over the sequence (SconeOcc.py:123-126).
 *
 * Leading dimensions and alignment (floats; checked on the host: a call outside them returns non-zero and writes nothing):
 *   every leading dimension must cover its row (ldx >= K or E, ldy / ldr >= N or E, 2 E for mcr_pool_max_avg's output,
 *   ldq >= 2 qk_dim + v_dim, ldo >= v_dim); rows may overlap nothing else: padding columns are neither read nor written.
 *   mcr_linear, mcr_layernorm, mcr_colmax_broadcast, mcr_pool_max_avg: any such leading dimension, operands 4-byte aligned
 *     (16-byte loads / stores are taken only where the operand's alignment and ld % 4 == 0 allow them; same values either way).
 *   mcr_attention, mcr_attention_ws: any ldq / ldo, operands 4-byte aligned; the matrix-pipe kernel needs qkv 16-byte aligned and
 *     ldq % 4 == 0, anything else (but 16-token sequences of the (32,128) layout, which have a kernel of their own) runs the
 *     slower scalar kernel (same reference, other summation order).
 *   mcr_attention_masked: as mcr_attention for 16-token sequences of the (32,128) layout; every other shape needs qkv 16-byte
 *     aligned and ldq % 4 == 0 (the mask exists on the matrix-pipe kernel alone) and is refused otherwise; out / ldo: any.
 *   mcr_attention_planes: ldq % 4 == 0, qkv and workspace 16-byte aligned (refused otherwise); out 4-byte aligned, any ldo. */
int mcr_linear(const float* X, int64_t ldx, const float* W, const float* bias, const float* residual, int64_t ldr, float* Y,
               int64_t ldy, int64_t M, int N, int K, int gelu, void* stream);
int mcr_layernorm(const float* X, int64_t ldx, const float* gamma, const float* beta, float* Y, int64_t ldy, int64_t M, int E,
                  void* stream);
int mcr_attention(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                  int v_dim, void* stream);
/* Same with a scratch buffer of mcr_attention_workspace_bytes(S, L, n_heads, v_dim) bytes: one or two long sequences (too few
 * blocks to fill the chip) split their keys over two blocks and merge the partial soft-maxes (results differ from mcr_attention
 * by summation order only, ~1e-6). */
size_t mcr_attention_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim);
int mcr_attention_ws(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                     int v_dim, void* workspace, size_t workspace_bytes, void* stream);
/* attention(q, k, v, mask) of Attention.py:8-36 WITH a mask (:24-27): where the mask byte of (sequence s, head h, query q, key k) --
 * mask[s * mask_seq_stride + h * mask_head_stride + q * mask_query_stride + k] -- is 0 the score is replaced by -1e3 BEFORE the
 * division by sqrt(d) (upstream's masked_fill rule: a fully masked query attends uniformly over the keys; it is not -inf).  Strides
 * of 0 broadcast: a [S, L] key mask has query and head stride 0, upstream's [S, 1, L, L] has head stride 0.  workspace: as
 * mcr_attention_ws (may be NULL).  fp32 P V (the fp16-split P V of the unmasked path is not taken). */
int mcr_attention_masked(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                         int v_dim, const unsigned char* mask, int64_t mask_seq_stride, int64_t mask_head_stride,
                         int64_t mask_query_stride, void* workspace, size_t workspace_bytes, void* stream);
/* The long-sequence attention of the encoders on the fp16-split matrix path (variant 6, sequences of >= 512 tokens), as one call: the
 * packed rows are split ONCE into fp16 hi/lo planes (inside the networks the QKV projection's epilogue writes them), K / V tiles then
 * reach LDS by DMA and both products run on fp16 pairs (attention_planes.hip).  Needs |q|, |k|, |v| < 65504 (an inf / NaN output tells).
 * lens (optional, device int per sequence): keys = the first min(L, lens[s]) rows.  split_mode: 1 = keys of every sequence over two
 * blocks (L >= 512), 0 = never, -1 = only when the unsplit grid leaves CUs idle.  workspace: mcr_attention_planes_workspace_bytes. */
size_t mcr_attention_planes_workspace_bytes(int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim);
int mcr_attention_planes(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                         int v_dim, const int* lens, int split_mode, void* workspace, size_t workspace_bytes, void* stream);
int mcr_colmax_broadcast(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, void* stream);
int mcr_pool_max_avg(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, void* stream);

/* ---- the padded-sequence forward as blocks: BRING-UP / TEST entries ------------------------------------------------------------------
 * The forms of the blocks above that the networks run on padded batches (the NBV step without a host sync, the ragged occupancy
 * pass): lens is a DEVICE int[S], sequence s takes part with its first n = min(L, max(1, lens[s])) rows; lens may be NULL (n = L).
 * The networks call the same launchers directly; these entries add no kernel.
 * mcr_attention_lens: mcr_attention with keys = the first n rows of the sequence (every one of the L query rows still gets an
 *   output; rows >= n are finite and otherwise unspecified).  split_mode as mcr_attention_planes (1: keys over two blocks whenever
 *   L >= 512; 0: never; -1: only when the unsplit grid leaves CUs idle); workspace: mcr_attention_workspace_bytes, 16-byte aligned;
 *   it may be NULL for split_mode 0 and -1 (never split then), a split_mode of 1 at L >= 512 without it, or any workspace too small
 *   for a split that the mode allows, is refused.  mcr_call_variant(1) selects the fp32 P V form.  lens exists on the matrix-pipe
 *   kernel alone: qkv 16-byte aligned and ldq % 4 == 0, refused otherwise (3); without lens as mcr_attention_ws.  S <= 32767
 *   (without lens: any S at L = 16).
 * mcr_pool_max_avg_lens: mcr_pool_max_avg over the first n rows: the max, and the mean as sum / n.
 * mcr_colmax_broadcast_lens: mcr_colmax_broadcast with the max over the first n rows, written to ALL L rows of the sequence.  ex
 *   (optional): columns 0 .. ex_cols - 1 of a second array [S * L, ex_ld] are copied to ex_dst [S * L, ldy] -- the leading dimension
 *   of Y -- on the way (all L rows); needs ex_dst, 0 < ex_cols <= ex_ld, ex_cols <= ldy, ex_ld < 2^31.  Without ex: ex_cols = 0,
 *   ex_dst NULL.
 * mcr_layernorm_planes: mcr_layernorm (eps 1e-5) with the result written as fp16 planes hi = fp16(y), lo = fp16(y - hi) [M, ldp]:
 *   the planes mcr_split_to_planes gives for mcr_layernorm's rows, bit for bit.  Yl may be NULL (the high plane alone).  E <= 512;
 *   E, ldx, ldp and alignment as mcr_split_to_planes (E % 4 == 0, ldx % 4 == 0, X 16-byte aligned, ldp % 4 == 0, planes 8-byte
 *   aligned); gamma, beta 4-byte aligned.
 * Leading dimensions and alignment otherwise as the entries without lens; a call outside them returns non-zero and writes nothing. */
int mcr_attention_lens(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                       const int* lens, int split_mode, void* workspace, size_t workspace_bytes, void* stream);
int mcr_pool_max_avg_lens(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, const int* lens, void* stream);
int mcr_colmax_broadcast_lens(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, const int* lens,
                              const float* ex, int64_t ex_ld, int ex_cols, float* ex_dst, void* stream);
int mcr_layernorm_planes(const float* X, int64_t ldx, const float* gamma, const float* beta, void* Yh, void* Yl, int64_t ldp, int64_t M,
                         int E, void* stream);

/* ---- the planes GEMMs of variants 6 / 7 as blocks (linear3p.hip): BRING-UP / TEST entries -----------------------------------------
 * The matrix path of the default numerics: both operands stored as fp16 planes, hi = fp16(x) (round to nearest even) and
 * lo = fp16(x - hi), and multiplied as W_lo X_hi + W_hi X_lo + W_hi X_hi in fp32 (n_planes = 2), or the high planes alone
 * (n_planes = 1, variant 7; Xl / Wl / Yl / Pl are then neither read nor written and may be NULL).  The networks call the same
 * launchers directly; these entries add no kernel.  hi and lo are independent operands: nothing assumes that lo came from a split.
 * mcr_split_to_planes: X [M, ldx] fp32 -> Ph, Pl [M, ldp] fp16, the first E columns of every row; Pl may be NULL.  Needs |x| < 65504
 *   (beyond it, and for inf / NaN, hi is non-finite -- what the range guard looks for).
 * mcr_linear_planes: y[m][n] = act(wscale_inv * sum_k W[n][k] X[m][k] + bias[n] + row_bias[g(m)][n]) (+ R[m][n], fp32 output only),
 *   X planes [M, ldx], W planes [N, ldw] (the weights times a power of two whose inverse is wscale_inv), bias [N] or NULL, row_bias
 *   [groups, N] or NULL with g(m) = row_group[m] (device int [M]) if row_group, else m / rows_per_group; act = the exact-erf GELU
 *   (gelu != 0; erf by Abramowitz-Stegun 7.1.26) or identity.  Exactly one of Y (fp32 [M, ldy]) and Yh (with Yl: y split into planes
 *   [M, ldy] again; n_planes = 1: Yh = fp16(y) alone) is given.  R may be Y (in place x += ...).  Which of the three tile forms runs
 *   follows from the shape alone (M <= 4096, no row bias, K = 128 or a multiple of 256: one shot; else K <= 512: two stages; else
 *   three); every form adds the same products in the same order, so the bits do not depend on it.
 * mcr_linear_planes_dot: out[m] = act2(sum_n act(y[m][n]) v[n] + c[0]) for a 256-feature layer (N = 256; y as above without row
 *   bias; c may be NULL), one launch for two layers; the 256 terms are added in one fixed order whatever M is.
 * Leading dimensions and alignment (checked on the host: a call outside them returns 1 and launches nothing).  Leading dimensions of
 *   planes are in halves, of fp32 operands in floats; every one must cover its row.
 *   mcr_split_to_planes: E % 4 == 0; ldx % 4 == 0 and X 16-byte aligned (16-byte loads); ldp % 4 == 0 and Ph, Pl 8-byte aligned.
 *   mcr_linear_planes, mcr_linear_planes_dot: K % 32 == 0; N % 4 == 0; ldx % 8 == 0, ldw % 8 == 0 and Xh, Xl, Wh, Wl 16-byte aligned
 *     (rows reach LDS by 16-byte DMA); bias, row_bias and v 16-byte aligned (read four columns at a time; row_bias rows have stride N);
 *     ldy % 4 == 0; Yh, Yl 8-byte aligned; Y, R, out, c 4-byte aligned, any ldr >= N.  Whole-row 16-byte stores are taken where N % 8
 *     == 0, ldy % 8 == 0 and 16-byte aligned planes (fp32: ldr % 4 == 0 and 16-byte aligned Y, R, no row bias) allow them, else a lane
 *     stores its own four columns; same values either way.  n_planes in {1, 2}; a residual needs fp32 output; row_bias needs
 *     rows_per_group > 0 or row_group. */
int mcr_split_to_planes(const float* X, int64_t ldx, void* Ph, void* Pl, int64_t ldp, int64_t M, int E, void* stream);
int mcr_linear_planes(const void* Xh, const void* Xl, int64_t ldx, const void* Wh, const void* Wl, int64_t ldw, const float* bias, float* Y,
                      void* Yh, void* Yl, int64_t ldy, int64_t M, int N, int K, int gelu, float wscale_inv, const float* row_bias,
                      int64_t rows_per_group, const int* row_group, const float* R, int64_t ldr, int n_planes, void* stream);
int mcr_linear_planes_dot(const void* Xh, const void* Xl, int64_t ldx, const void* Wh, const void* Wl, int64_t ldw, const float* bias,
                          int64_t M, int K, int gelu, float wscale_inv, const float* v, const float* c, int gelu2, float* out,
                          int n_planes, void* stream);

/* ---- backward building blocks (bwd_blocks.hip, attention_bwd.hip): fp32, deterministic (no float atomics; fixed-order sums) ----------------------
 * mcr_attention_backward: gradient of mcr_attention's output (with lens as mcr_attention_planes: keys of sequence s = its first
 *   min(L, max(1, lens[s])) rows; lens may be NULL) with respect to the packed rows: d_qkv [S*L, ld_dqkv] <- [dq | dk | dv] given
 *   d_out [S*L, ld_dout].  Per-head widths 16 (q, k) and 64 (v) only.  The forward is recomputed (O and the log-sum-exp of every
 *   (row, head)); P is rebuilt tile by tile and never stored.  Keys no query attends to get a zero gradient.  Leading dimensions
 *   multiples of 4, operands 16-byte aligned.  workspace: mcr_attention_backward_workspace_bytes(S, L, n_heads, v_dim).
 * mcr_linear_backward: for Y = act(X W^T + b), act = exact-erf GELU (gelu != 0; Z = the pre-activation X W^T + b, [M, N] with
 *   leading dimension ldz) or identity (Z unused): dX[M, K] = dZ W (added to dX when accumulate_dx, else written), dW[N, K] = dZ^T X,
 *   db[N] = sum over rows of dZ, dZ = dY * act'(Z).  dX, dW, db may each be NULL.  workspace: mcr_linear_backward_workspace_bytes.
 * mcr_layernorm_backward: for Y = LayerNorm(X) (eps 1e-5): dX (+)= the input gradient, d_gamma, d_beta [E] (each may be NULL).
 *   E in {64, 128, 256, 512}.  workspace: mcr_layernorm_backward_workspace_bytes(M, E).
 * mcr_colmax_backward: for mcr_colmax_broadcast (lens as above, may be NULL: the max over the first lens[s] rows): for every
 *   (sequence, column c < E) dX[row*, c] += sum over ALL L rows of d_bcast[row, c], row* = the lowest valid row holding the max
 *   (torch.max(dim)'s choice on ties).
 * Leading dimensions and alignment (checked on the host: a call outside them returns non-zero and writes nothing): every leading
 *   dimension must cover its row.  mcr_attention_backward: ldq, ld_dout, ld_dqkv multiples of 4; qkv, d_out, d_qkv and workspace
 *   16-byte aligned.  mcr_linear_backward, mcr_layernorm_backward, mcr_colmax_backward: any leading dimension >= the row, operands
 *   and workspace 4-byte aligned (scalar accesses throughout).  mcr_linear_backward reads X for db as well as for dW (db rides on
 *   the dW product): X may be NULL only when both are.
 * mcr_attention_backward_pct: mcr_attention_backward for the PCTransformer's heads: 4 heads of per-head widths 8 (q, k) and 32 (v),
 *   packed rows [q 32 | k 32 | v 128], scores / sqrt(8); same arguments, leading dimensions and alignment.  L == 16 (any S): one wave
 *   per sequence rebuilds the soft-max in registers and writes d_qkv alone -- no workspace is touched (workspace may be NULL), and
 *   lens must be NULL (refused otherwise).  Any other L: the recomputing three-pass scheme above, S <= 65535, lens honoured.
 *   workspace: mcr_attention_backward_pct_workspace_bytes(S, L).
 * mcr_pool_max_avg_backward: for mcr_pool_max_avg given dY [S, ldy] = [d_max (E) | d_avg (E)]: dX[(s, r), c] = d_avg[s, c] / L, plus
 *   d_max[s, c] on the lowest row r holding the column's max (torch.max(dim)'s choice on ties).  Written, not accumulated.  Any S;
 *   leading dimensions >= the row (ldy >= 2 E), operands 4-byte aligned.
 * mcr_pool_max_avg_backward_lens: the same for padded sequences (the backward of mcr_pool_max_avg_lens; lens: DEVICE int[S]): with n = min(L,
 *   max(1, lens[s])) the arg-max runs over the first n rows (ties: the lowest row), the mean's share is d_avg / n, and rows >= n are
 *   written as exact zeros. */
size_t mcr_attention_backward_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim);
int mcr_attention_backward(const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                           int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes,
                           void* stream);
size_t mcr_linear_backward_workspace_bytes(int64_t M, int N, int K);
int mcr_linear_backward(const float* X, int64_t ldx, const float* W, const float* Z, int64_t ldz, const float* dY, int64_t ldy, int64_t M,
                        int N, int K, int gelu, float* dX, int64_t ld_dx, int accumulate_dx, float* dW, float* db, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t mcr_layernorm_backward_workspace_bytes(int64_t M, int E);
int mcr_layernorm_backward(const float* X, int64_t ldx, const float* gamma, const float* dY, int64_t ldy, int64_t M, int E, float* dX,
                           int64_t ld_dx, int accumulate_dx, float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes,
                           void* stream);
int mcr_colmax_backward(const float* X, int64_t ldx, const float* d_bcast, int64_t ldg, float* dX, int64_t ld_dx, int64_t S, int64_t L,
                        int E, const int* lens, void* stream);
size_t mcr_attention_backward_pct_workspace_bytes(int64_t S, int64_t L);
int mcr_attention_backward_pct(const float* qkv, int64_t ldq, const float* d_out, int64_t ld_dout, float* d_qkv, int64_t ld_dqkv, int64_t S,
                               int64_t L, int n_heads, int qk_dim, int v_dim, const int* lens, void* workspace, size_t workspace_bytes,
                               void* stream);
int mcr_pool_max_avg_backward(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S, int64_t L,
                              int E, void* stream);
int mcr_pool_max_avg_backward_lens(const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ld_dx, int64_t S,
                                   int64_t L, int E, const int* lens, void* stream);

/* ---- network forwards -----------------------------------------------------------------------------------
 * Weight tables are arrays of device pointers to contiguous fp32 tensors in nn.Module layout ([out,in] weights):
 *   ENCODER (12): norm1.weight, norm1.bias, qkv.weight, qkv.bias, out.weight, out.bias, norm2.weight, norm2.bias,
 *                 ff.linear1.weight, ff.linear1.bias, ff.linear2.weight, ff.linear2.bias
 *                 where qkv = rows of mhsa.w_q, mhsa.w_k, mhsa.w_v stacked ([2*qk_dim + E, E]) and likewise the bias.
 *   PCT (32):     embedding.linear1.{weight,bias}, embedding.linear2.{weight,bias}, ENCODER x2, norm.{weight,bias},
 *                 linear0.{weight,bias}
 *   SCONE_VIS (48): embedding.linear1.{w,b}, embedding.linear2.{w,b}, ENCODER x3, norm.{w,b}, fc1.{w,b}, fc2.{w,b}, fc3.{w,b}
 *   SCONE_OCC (140): PCT global_transformer, PCT local_transformers.{0,1,2}, x_embedding.linear{1,2,3}.{w,b},
 *                 linear1.{w,b}, linear2.{w,b}, linear3.{w,b}
 *   PLANES (optional tail; n_weights = 32 + 8 / 48 + 12 / 140 + 8): per ENCODER of the long-sequence networks (PCT's two, SCONE_VIS's
 *                 three, SCONE_OCC's global_transformer's two) four more pointers -- qkv.weight, out.weight, ff.linear1.weight,
 *                 ff.linear2.weight as fp16 hi/lo planes [2][N][K] of W * 2^8 (hi = fp16(x), lo = fp16(x - hi);
 *                 networks/packing.py: encoder_weight_planes) -- for the planes GEMMs of variant 6 (sequences of >= 512 tokens).
 *                 Without the tail the weights are split by one small launch per GEMM and call.
 *   END PLANES (optional, behind PLANES; n_weights = 32 + 11 / 48 + 17 / 140 + 11): the layers either side of the encoders on the same
 *                 path -- PCT / SCONE_OCC's global_transformer: embedding.linear2.weight zero-padded to planes [2][128][128],
 *                 its bias zero-padded to fp32 [128], linear0.weight planes; SCONE_VIS: the same two for its embedding.linear2
 *                 (126 x 126 -> 128 x 128), then fc1, fc2, fc3 planes (networks/packing.py: padded_weight_planes, weight_planes).
 *
 * mcr_pc_transformer_forward: PCTransformer.forward (macarons/networks/SconeOcc.py:104-130); pc [S,L,3] ->
 *   features [S, feature_dim] (max || avg), feature_dim in {256, 512}.
 * mcr_scone_vis_forward: SconeVis.forward (macarons/networks/SconeVis.py:121-162); pts [B,N,4], view_harmonics
 *   [B,N,64] -> out [B,N,64].  Default architecture only (pts_embedding_dim 256, 4 heads, 3 encoders,
 *   view_state_mode "end", global feature, concatenated input).  lengths (optional, DEVICE int32 [B], may be NULL): cloud b
 *   consists of its first min(N, lengths[b]) rows only -- the cloud-wide max of the embedding and the attention keys stop
 *   there; rows beyond still produce (meaningless) outputs.  This is how the padded output of mcr_sample_proxy is consumed
 *   without its count ever reaching the host (the reference slices with the count on the host, testers/shapenet.py:146-157).
 * mcr_scone_occ_forward: SconeOcc.forward (macarons/networks/SconeOcc.py:250-347) given the clouds the reference
 *   would obtain from its torch.randperm draws (:269, :311), which the HOST performs so the RNG stream matches:
 *   pc_global [B,Lg,3]; pc_scale[i] [B,M_scale[i],3] for the 3 neighbourhood scales; x [B,Q,3];
 *   view_harmonics [B,Q,64] -> out [B,Q,1].  pc_scale / M_scale are HOST arrays of 3 entries.
 *   head_planes / head_inv_scales (optional, HOST arrays of 4; variant 6 only): the fp16 hi/lo planes of the four large head
 *   matrices -- x_embedding.linear2 [256,128], x_embedding.linear3 [512,256], linear1[:, 512:1856] [512,1344], linear2
 *   [256,512] -- each times a power of two 2^e, laid out [plane][n][K/8][8 fp16], and 2^-e (networks/packing.py:
 *   pack_head_planes); NULL: the kernel splits the weights itself on every call (fixed 2^8 scale: needs |w| < 255).
 *   range_flag (optional, DEVICE int, cleared by the caller): set to 1 when an occupancy comes out non-finite -- on the fp16
 *   split path (variant 6, |activation| < 65504) that is what an out-of-range activation turns into; the host mirror then
 *   re-runs the call on variant 5 (whole fp32 range). */
size_t mcr_pc_transformer_workspace_bytes(int64_t S, int64_t L);
int mcr_pc_transformer_forward(const float* pc, float* features, int64_t S, int64_t L, int feature_dim,
                               const float* const* weights, int n_weights, void* workspace, size_t workspace_bytes,
                               void* stream);
size_t mcr_scone_vis_workspace_bytes(int64_t B, int64_t N);
int mcr_scone_vis_forward(const float* pts, const float* view_harmonics, float* out, int64_t B, int64_t N,
                          const float* const* weights, int n_weights, const int* lengths, void* workspace,
                          size_t workspace_bytes, void* stream);
/* mcr_scone_vis_backward: gradient of mcr_scone_vis_forward (same arguments) given d_out [B,N,64], computed on the fp32 network
 *   whatever the call's variant (on variants 6 and 7 it is the gradient of the fp32 network at the same inputs; the fp16 planes
 *   path is never used, so no range guard applies).  The forward is recomputed: the residual stream at the four encoder boundaries
 *   and the embedding / head pre-activations are kept, each encoder's interior is rebuilt just before its backward.
 *   weights: the SCONE_VIS table (48 entries; a PLANES / END PLANES tail is accepted and ignored).
 *   d_weights (may be NULL: no parameter gradients): 48 DEVICE pointers in the table's order and shapes (the packed qkv weight
 *   [384,256] and bias [384] one entry each); written, not accumulated.  d_pts [B,N,4] and d_view_harmonics [B,N,64] may be NULL.
 *   lengths: as the forward; padded rows keep their outputs and their upstream gradient flows like any other row's.
 *   workspace: mcr_scone_vis_backward_workspace_bytes(B, N) bytes.  Deterministic (no float atomics), no host synchronisation. */
size_t mcr_scone_vis_backward_workspace_bytes(int64_t B, int64_t N);
int mcr_scone_vis_backward(const float* pts, const float* view_harmonics, const float* d_out, int64_t B, int64_t N,
                           const float* const* weights, int n_weights, const int* lengths, float* const* d_weights, float* d_pts,
                           float* d_view_harmonics, void* workspace, size_t workspace_bytes, void* stream);
/* mcr_pc_transformer_backward: gradient of mcr_pc_transformer_forward given d_features [S, feature_dim], computed on the fp32 network
 *   whatever the call's variant (as mcr_scone_vis_backward).  The forward is recomputed: the residual stream at the three encoder
 *   boundaries and the embedding's pre-activation are kept, each encoder's interior is rebuilt just before its backward.
 *   weights: the PCT table (32 entries; a PLANES / END PLANES tail is accepted and ignored).
 *   d_weights (may be NULL: no parameter gradients): 32 DEVICE pointers in the table's order and shapes (the packed qkv weight
 *   [192,128] and bias [192] one entry each); written, not accumulated.  d_pc [S,L,3] may be NULL; both NULL: returns 0 at once.
 *   L == 16 || S <= 65535, as the forward.  Sequences of 16 tokens are processed INSIDE the entry in chunks of
 *   mcr_pc_transformer_backward_chunk(S, L) sequences -- a function of (S, L) alone -- whose weight gradients are summed in chunk
 *   order, so the workspace does not grow with S beyond one chunk and two calls give identical bits; other lengths run as one chunk.
 *   pc, d_features and the workspace 16-byte aligned.  workspace: mcr_pc_transformer_backward_workspace_bytes(S, L) bytes.
 *   Deterministic (no float atomics), no host synchronisation. */
int mcr_pc_transformer_backward_chunk(int64_t S, int64_t L);
size_t mcr_pc_transformer_backward_workspace_bytes(int64_t S, int64_t L);
int mcr_pc_transformer_backward(const float* pc, const float* d_features, int64_t S, int64_t L, int feature_dim,
                                const float* const* weights, int n_weights, float* const* d_weights, float* d_pc, void* workspace,
                                size_t workspace_bytes, void* stream);
/* mcr_scone_occ_backward: gradient of mcr_scone_occ_forward given d_out [B,Q,1] and the neighbour selection, computed on the fp32
 *   network whatever the call's variant (as mcr_scone_vis_backward: no fp16 plane is used, no range guard applies).
 *   pc_global, Lg, pc_scale, M_scale (HOST arrays of 3, every M_scale[i] >= 16), x, view_harmonics, weights: as the forward; weights is the
 *   SCONE_OCC table (140 entries; the PLANES / END PLANES tails are accepted and ignored).
 *   knn_idx: HOST array of 3 DEVICE pointers to int64 [B,Q,16], the 16 nearest points of pc_scale[i][b] of every query (what the
 *   forward's search selects; an index outside [0, M_scale[i]) is clamped into the cloud).  The selection carries no gradient.
 *   d_weights (may be NULL: no parameter gradients): 140 DEVICE pointers in the table's order and shapes (every transformer's packed qkv
 *   weight [192,128] and bias [192] one entry each); written, not accumulated.  d_x [B,Q,3] and d_view_harmonics [B,Q,64] may be NULL;
 *   all three NULL: returns 0 at once.  There is no gradient for the surface points.
 *   The global transformer's forward runs once; then, cloud by cloud, the queries are processed in chunks of q_chunk rows (0: the default,
 *   mcr_scone_occ_backward_chunk(Q) = the 16-token chunk of mcr_pc_transformer_backward; else a multiple of 16, >= 16; a chunk never
 *   crosses a cloud): gather, local transformers, x embedding and head forward, then their backward; the chunks' weight gradients and their
 *   shares of the global features' gradient are summed in chunk order; the global transformer's backward runs last.  The workspace holds
 *   one chunk whatever Q is.  Two calls give identical bits; the bits may depend on q_chunk (another summation order of the chunks).
 *   pc_global, pc_scale[i], knn_idx[i], x, view_harmonics, d_out, the outputs and the workspace 16-byte aligned.
 *   workspace: mcr_scone_occ_backward_workspace_bytes(B, Q, Lg, q_chunk) bytes.  Deterministic (no float atomics), no host
 *   synchronisation. */
int mcr_scone_occ_backward_chunk(int64_t Q);
size_t mcr_scone_occ_backward_workspace_bytes(int64_t B, int64_t Q, int64_t Lg, int64_t q_chunk);
int mcr_scone_occ_backward(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale, const float* x,
                           const float* view_harmonics, const int64_t* const* knn_idx, const float* d_out, int64_t B, int64_t Q,
                           const float* const* weights, int n_weights, float* const* d_weights, float* d_x, float* d_view_harmonics,
                           int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream);
/* mcr_scone_occ_backward_ragged: the gradient of J independent mcr_scone_occ_forward calls of different sizes (the jobs of the ragged
 *   occupancy pass) given d_out [T], T = the jobs' query rows one behind the other; weight gradients summed over the jobs.  Computed on
 *   the fp32 network whatever the call's variant; no gradient for any cloud.
 *   pc_global [J,Lg,3]: every job's global sequence padded to Lg rows, global_len (DEVICE int[J]): its valid rows, n = min(Lg,
 *   max(1, global_len[j])) -- keys >= n are masked, the pooling runs over the first n rows (mean divided by n).  What the padding rows
 *   hold is never used (NaN included): the entry works on a copy whose padding is the sequence's row 0.  Lg == 16 is refused.
 *   offsets: HOST array of 3 DEVICE pointers to [T,16,3], the neighbourhoods of every query row and scale as neighbour minus query (what
 *   mcr_knn_offsets_segmented writes): the entry takes no clouds and no indices.  The selection carries no gradient; the query's share
 *   of the offsets' gradient goes to d_x.
 *   x [T,3], view_harmonics [T,64]; row_job (DEVICE int[T], non-decreasing): the job of every row (a value outside [0, J) is clamped);
 *   job_rows (DEVICE int64[J+1]): job j = rows [job_rows[j], job_rows[j+1]) (clamped into [0, T]); the two must agree.  A job may have
 *   no rows: its sequence then contributes exact zeros.
 *   weights, d_weights (may be NULL), d_x [T,3] and d_view_harmonics [T,64] (may be NULL; all three NULL: returns 0 at once): as
 *   mcr_scone_occ_backward.
 *   Schedule: the global transformer's forward over the J padded sequences; then the rows [0, T) in chunks of q_chunk rows (0: the
 *   default, mcr_scone_occ_backward_chunk(T); else a multiple of 16 in [16, 2^20]) -- a chunk may span any number of jobs -- each running
 *   local transformers, x embedding and head forward and backward as mcr_scone_occ_backward does, the chunks' weight gradients summed in
 *   chunk order, each job's share of the global features' gradient summed in row order; then the global transformer's backward job by
 *   job, summed in job order (one job's share depends on that job alone: adding or removing a job without rows changes no bit).
 *   Two calls give identical bits; the bits may depend on q_chunk.
 *   Workspace: mcr_scone_occ_backward_ragged_workspace_bytes(J, T, Lg, q_chunk) bytes: one chunk of rows whatever T is, plus the J global
 *   sequences' forward OVER the chunk's scratch, so beyond the chunk's size it is linear in J (at Lg = 2048: the 681 MB of a 2048-row
 *   chunk up to J = 29, about 23 MB per job beyond); J <= 16384 (refused beyond; the global sequences are not processed in groups).
 *   pc_global, offsets[i], x, view_harmonics, d_out, the outputs and the workspace 16-byte aligned.  Deterministic (no float
 *   atomics), no host synchronisation, no read-back. */
size_t mcr_scone_occ_backward_ragged_workspace_bytes(int64_t J, int64_t T, int64_t Lg, int64_t q_chunk);
int mcr_scone_occ_backward_ragged(const float* pc_global, const int* global_len, int64_t Lg, const float* const* offsets, const float* x,
                                  const float* view_harmonics, const int* row_job, const int64_t* job_rows, const float* d_out, int64_t J,
                                  int64_t T, const float* const* weights, int n_weights, float* const* d_weights, float* d_x,
                                  float* d_view_harmonics, int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream);
size_t mcr_scone_occ_workspace_bytes(int64_t B, int64_t Q, int64_t Lg);
int mcr_scone_occ_forward(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale,
                          const float* x, const float* view_harmonics, float* out, int64_t B, int64_t Q,
                          const float* const* weights, int n_weights, const float* const* local_blobs,
                          const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                          size_t workspace_bytes, void* stream);

/* mcr_scone_occ_forward in two calls on one stream and one workspace (phase 0 = the single call).
 *   phase 1: what needs neither view_harmonics nor a hidden draw -- the query order of the grid search and scale 0 (the whole
 *            cloud: k-NN + local transformer).  Reads x, pc_scale[0], M_scale[0..2]; pc_global, pc_scale[1..2], view_harmonics and
 *            out may be NULL.  It is the first long kernel of an NBV step (testers/shapenet.py:126-144): queued before the host builds
 *            the view state, the harmonics and the down-sampled clouds, it hides their launch latency.
 *   phase 2: the rest (global transformer, scales 1 and 2, x embedding, head) -> out; same arguments as the single call. */
int mcr_scone_occ_forward_phase(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale,
                                const float* x, const float* view_harmonics, float* out, int64_t B, int64_t Q,
                                const float* const* weights, int n_weights, const float* const* local_blobs,
                                const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                size_t workspace_bytes, int phase, void* stream);

/* Ragged SconeOcc: J independent SconeOcc.forward calls ("jobs" = one surface cloud + one chunk of queries, all of different
 * sizes: the per-cell passes of compute_scene_occupancy_probability_field, macarons/utility/macarons_utils.py:1395-1540, which
 * upstream runs one after the other from a Python loop over the grid cells) in ONE launch sequence.
 *   pc_global [J,Lg,3]: job j's global down-sample (its first global_len[j] rows; the rest padding), global_len DEVICE int[J];
 *   pc_scale[s] (HOST array of 3 device pointers): the neighbourhood clouds of scale s of all jobs back to back, job j =
 *     rows [scale_off[s][j], scale_off[s][j+1]) (scale_off: HOST array of 3 DEVICE int64[J+1]); every job needs >= 16 points per scale;
 *   x [T,3], view_harmonics [T,64]: the queries of all jobs back to back, sorted by job; row_job DEVICE int[T];
 *   knn_blocks DEVICE int[n_blocks*4] = (job, first row, rows <= mcr_knn_rows_per_block(), 0) per workgroup of the segmented
 *     kNN, covering every row exactly once;  out [T].  Needs the fused local-transformer blobs; other arguments as above. */
int mcr_knn_rows_per_block(void);
size_t mcr_scone_occ_ragged_workspace_bytes(int64_t J, int64_t T, int64_t Lg);
int mcr_scone_occ_forward_ragged(const float* pc_global, const int* global_len, int64_t Lg, const float* const* pc_scale,
                                 const int64_t* const* scale_off, const float* x, const float* view_harmonics, const int* row_job,
                                 const int* knn_blocks, int64_t n_blocks, float* out, int64_t J, int64_t T,
                                 const float* const* weights, int n_weights, const float* const* local_blobs,
                                 const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The same as two calls on one stream with ONE workspace: phase 1 = what needs none of the hidden torch.randperm draws (the scale-0
 * search and local transformer over the whole clouds; the x embedding on the fp16-planes path) -- it reads pc_scale[0], scale_off[0],
 * x, view_harmonics, row_job, knn_blocks, local_blobs[0] only (the other arrays may hold anything, pc_global / global_len / out may be
 * NULL); phase 2 = the rest.  The host makes the draws between the two calls while the GPU works on phase 1 (a MACARONS decision
 * otherwise idles ~2.5 ms there).  phase 0 = both = mcr_scone_occ_forward_ragged. */
int mcr_scone_occ_forward_ragged_phase(const float* pc_global, const int* global_len, int64_t Lg, const float* const* pc_scale,
                                       const int64_t* const* scale_off, const float* x, const float* view_harmonics, const int* row_job,
                                       const int* knn_blocks, int64_t n_blocks, float* out, int64_t J, int64_t T,
                                       const float* const* weights, int n_weights, const float* const* local_blobs,
                                       const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                       size_t workspace_bytes, int phase, void* stream);

/* Fused per-query local PCTransformer (the FLOP majority of SconeOcc.forward, SconeOcc.py:293-304 + :104-130):
 *   offsets [S,16,3] (kNN neighbours minus the query) -> features[s*ld_features + 0:256] = max(128) || avg(128).
 * `blob`: 16-byte-aligned device image of ONE local transformer's parameters, mcr_local_pct_blob_floats() floats,
 * laid out as macarons_amd/networks/packing.py builds it (MFMA-fragment order, LayerNorm folded into the
 * following linear layer).  mcr_scone_occ_forward uses the fused kernel for scale i when local_blobs != NULL and
 * local_blobs[i] != NULL (HOST array of 3 device pointers), else the layer-by-layer path. */
int mcr_local_pct_blob_floats(void);
int mcr_local_pct3_blob_floats(void);
int mcr_local_pct6_blob_floats(void);
int mcr_local_pct7_blob_floats(void);
/* Kernel variant behind mcr_local_pct_forward / the fused path of mcr_scone_occ_forward.  The blob must have been packed
 * for the selected variant (macarons_amd/networks/packing.py):
 *   1: exact-fp32 MFMA, one workgroup/CU (local_pct.hip; mcr_local_pct_blob_floats() floats);
 *   5: split precision, every fp32 operand as exact bf16 hi/mid/lo, six MFMAs per product, two workgroups per CU, valid
 *      for the whole fp32 range (local_pct5.hip; mcr_local_pct3_blob_floats() floats);
 *   6 (default): two-term fp16 split (hi + lo, 22 significant bits), three MFMAs per product, same structure
 *      (local_pct6.hip; mcr_local_pct6_blob_floats() floats); needs |activation| < 65504;
 *   7 (OPT-IN, per call only: mcr_call_variant(7); mcr_set_local_pct_variant refuses it): BASELINE.json config 3's 16-bit matrix
 *      path -- ONE fp16 plane per matrix operand, one MFMA per product, fp32 accumulation; LayerNorm statistics, soft-max, GELU,
 *      pooling, SH math and every reduction stay fp32 (local_pct7.hip; mcr_local_pct7_blob_floats() floats; the SconeOcc head's
 *      planes GEMMs read the high planes alone).  NOT within the 1e-4 of variants 1 / 5 / 6: the bound on the occupancies is a
 *      property of (path, weight set) and is stated per weight set -- relative, against the fp64 oracle: 2e-3 on the golden
 *      weights (seed 2; measured 1.0e-3) and on seed 11, 8e-3 on seed 7 (measured 4.7e-3), 6e-3 on seed 2 with the local matrices
 *      x 4 (measured 3.5e-3): OCC_TOL_BY_WEIGHTS in tests/test_variant7_gpu.py; same range rule as variant 6. */
/* The variant is a property of a CALL: mcr_call_variant(v) is the per-call argument -- the NEXT network entry point (mcr_linear,
 * mcr_attention*, mcr_local_pct_forward, mcr_pc_transformer_forward, mcr_scone_vis_forward, mcr_scone_occ_forward*) called on THIS
 * thread runs on variant v (one-shot, thread-local; 0 = the default again).  mcr_set_local_pct_variant only sets the process DEFAULT
 * (start-up value: env MCR_LOCAL_PCT_VARIANT, else 6) that calls without a one-shot take; no call ever changes it. */
int mcr_set_local_pct_variant(int variant);
int mcr_get_local_pct_variant(void);
int mcr_call_variant(int variant);
/* Range guard of variant 6 for outputs that leave through an entry point without a flag argument (mcr_scone_vis_forward's harmonics):
 * *flag |= 1 if any of x[0 .. n) is inf / NaN -- what an activation beyond the fp16 range of the split matrix path turns into.  On
 * variant 6 the encoders of sequences of >= 512 tokens (SconeVis, SconeOcc's global transformer; Attention.py:278-300) run their
 * GEMMs on fp16 hi/lo planes (LayerNorm / GELU epilogues write the planes, operands reach LDS by DMA; env MCR_ENC_PLANES=0: the
 * full-range bf16 x 6 kernels of variant 5). */
int mcr_nonfinite_flag(const float* x, int64_t n, int* flag, void* stream);
/* mcr_local_pct_forward accepts: S > 0 sequences; any ld_features >= 256 (the row stride of `features` in floats: production writes
 * the three scales into columns 0, 256 and 512 of rows of 1344 floats); `offsets` [S,16,3] packed and `features` 4-byte aligned
 * (neither needs more); `blob` 16-byte aligned and packed for the variant of the call.  It writes features[s * ld_features + 0 .. 255]
 * for s < S and nothing else: rows >= S and the columns outside the 256 are never written, `offsets` is only read.  On variant 6
 * |offset| < 255 (the offsets are split as 2^8 x; beyond it the features come out non-finite).  Refused (non-zero, nothing launched):
 * a null pointer, S <= 0, ld_features < 256, a blob off the 16-byte grid.  Tested on guarded operands in tests/test_local_pct_gpu.py. */
int mcr_local_pct_forward(const float* offsets, float* features, int64_t ld_features, int64_t S, const float* blob,
                          void* stream);

/* ---- glue either side of the networks --------------------------------------------------------
 * mcr_view_state: compute_view_state (macarons/utility/scone_utils.py:799-860): for every (point, view) the
 *   elevation/azimuth of (X_view[v] - pts[p,:3]) is binned on the n_elev x n_azim lattice with the reference's
 *   exact clamp / wrap rules; view_state [n_points, n_elev*n_azim] fp32 0/1 (zeroed here, then set).
 * mcr_sample_proxy: sample_proxy_points (scone_utils.py:1030-1061) with the uniforms `u` supplied by the host:
 *   keeps points with preds > min_occ, draws n_sample points with probability proportional to preds (inverse
 *   CDF in fp64: first i with C_i >= u * C_last), then unique (sorted) + inverse.  Outputs are padded to
 *   n_sample rows (rows >= *n_unique are zero-filled); *n_unique (device int) says how many are valid.  uniq holds
 *   ORIGINAL point indices.  view_harmonics may be NULL (then res_harmonics is not written: a caller that only holds a
 *   shard of the harmonics recomputes the rows of the sampled points from uniq).  Three launches: block sums + scan of them by the last block to finish, one wave per sample
 *   for the search, one block for sort / unique / inverse / gather.
 *   res [n_sample,4] = (X, pred), res_harmonics [n_sample,64].  preds may be strided (pred_stride floats).
 *   volume (optional device double): sum of the kept occupancies (fov_proxy_volume of macarons_utils.py:1620).
 * mcr_points_in_fov: Camera.get_points_in_fov (macarons/utility/macarons_utils.py:2400-2435) for n_cam cameras
 *   at once.  Each camera is 40 floats: M_view[16] and M_proj[16] (row-major 4x4, row-vector convention
 *   p' = [x y z 1] M, as pytorch3d's get_world_to_view_transform / get_full_projection_transform matrices),
 *   {min_ndc_x, max_ndc_x, min_ndc_y, max_ndc_y}, camera centre[3], range (<= 0: no range test).
 *   mask [n_cam, P] bytes (0/1).
 * mcr_coverage_gain_multiple: the tuple stage of SconeVis.compute_coverage_gain_multiple (SconeVis.py:289-301):
 *   vis [B,C,N] -> gains [B, C^n_cam] over ordered tuples in torch.cartesian_prod order, n_cam in {2,3}. */
int mcr_view_state(const float* pts, int pts_dim, const float* X_view, float* view_state, int64_t n_points, int n_view,
                   int n_elev, int n_azim, void* stream);
/* Batched / in-place form.  n_clouds clouds of pts_per_cloud points each; cloud c is binned against ITS OWN view positions
 * X_view[c] ([n_clouds, n_view, 3]: every object of a scene batch has its own trajectory, testers/shapenet.py:33-37).
 * accumulate != 0: view_state is not cleared first -- bins are OR'ed into the caller's 0/1 table, which is what the reference's
 * `view_states[mask] += compute_view_state(...)` followed by torch.heaviside(., 0) does (macarons_utils.py:2867-2877); with
 * rows != NULL (device int64 [n_clouds*pts_per_cloud], needs accumulate) point p updates row rows[p] of the table, i.e. the
 * masked in-place update of the scene-wide state table in one launch. */
int mcr_view_state_batched(const float* pts, int pts_dim, const float* X_view, float* view_state, int64_t n_clouds,
                           int64_t pts_per_cloud, int n_view, int n_elev, int n_azim, const int64_t* rows, int accumulate,
                           void* stream);
size_t mcr_sample_proxy_workspace_bytes(int64_t P, int n_sample);
int mcr_sample_proxy(const float* X, const float* preds, int64_t pred_stride, const float* view_harmonics, int64_t P,
                     float min_occ, const float* u, int n_sample, float* res, float* res_harmonics, int64_t* uniq,
                     int64_t* inverse, int* n_unique, double* volume, void* workspace, size_t workspace_bytes, void* stream);
/* The same for B independent clouds in one launch sequence (a scene batch: every tensor gains a leading B; preds is
 * [B, P] with element stride pred_stride; u [B, n_sample]; n_unique int[B]; volume double[B] or NULL): every cloud draws from its
 * own CDF with its own uniforms, exactly as B calls of mcr_sample_proxy would. */
size_t mcr_sample_proxy_batched_workspace_bytes(int64_t B, int64_t P, int n_sample);
int mcr_sample_proxy_batched(const float* X, const float* preds, int64_t pred_stride, const float* view_harmonics, int64_t B,
                             int64_t P, float min_occ, const float* u, int n_sample, float* res, float* res_harmonics,
                             int64_t* uniq, int64_t* inverse, int* n_unique, double* volume, void* workspace,
                             size_t workspace_bytes, void* stream);
/* B distributions over ONE shared point set: X [P,3] and view_harmonics [P,64] are common, only preds [B,P] and u [B,n_sample]
 * differ -- the K neighbour cameras of a MACARONS decision, each sampling the scene's proxy points inside its own frustum
 * (preds = mcr_fov_mask_occ rows; macarons_utils.py:1603-1624).  Workspace as for the batched form. */
int mcr_sample_proxy_shared(const float* X, const float* preds, int64_t pred_stride, const float* view_harmonics, int64_t B,
                            int64_t P, float min_occ, const float* u, int n_sample, float* res, float* res_harmonics,
                            int64_t* uniq, int64_t* inverse, int* n_unique, double* volume, void* workspace,
                            size_t workspace_bytes, void* stream);
int mcr_points_in_fov(const float* pts, int64_t P, const float* cameras, int n_cam, unsigned char* mask, void* stream);
/* filter_proxy_points (macarons/utility/scone_utils.py:1001-1027; call site testers/shapenet.py:122): mask[p] = 1 iff in every
 * view v the projection ([x y z 1] * proj[v])[:2] / w of X[p] lies strictly inside the bounding box of the projected surface
 * cloud pc grown by filter_tol.  proj = n_view row-major 4x4 full-projection matrices (row-vector convention, as
 * pytorch3d's get_full_projection_transform().get_matrix()); bounds = n_view*4 floats of scratch, left holding
 * {min_x, max_x, min_y, max_y} per view. */
/* Column gather of move_view_state_to_view_space (macarons/utility/scone_utils.py:863-931, line :928; callers
 * macarons_utils.py:1356,1488): out[r, v] = in[r, idx[v]]; idx = the V bin indices the host derives from the camera rotation
 * (device int32, every entry in [0, V)). */
int mcr_gather_columns(const float* in, const int* idx, float* out, int64_t rows, int V, void* stream);
int mcr_filter_proxy_points(const float* X, int64_t P, const float* pc, int64_t M, const float* proj, int n_view, float filter_tol,
                            float* bounds, unsigned char* mask, void* stream);
int mcr_coverage_gain_multiple(const float* vis, float* gains, int64_t B, int64_t C, int64_t N, int n_cam, void* stream);

/* The end of a single-rank NBV decision in one launch: gains [B,C] (in/out) -> max_gain [B], nbv_idx [B] (int64), torch.max over
 * the cameras (testers/shapenet.py:172: first maximum, NaN wins); a cloud with n_unique[b] < 1 (nothing sampled: the reference
 * fails there, scone_utils.py:1052-1061) gets NaN gains, a NaN maximum and index -1.  n_unique / range_flag may be NULL.
 * record: 1 + 2 B doubles = (*range_flag or 0, nbv_idx[0..B), max_gain[0..B)) -- the one buffer a caller reads back. */
int mcr_nbv_decide(float* gains, int64_t B, int64_t C, const int* n_unique, const int* range_flag, float* max_gain, int64_t* nbv_idx,
                   double* record, void* stream);

/* Arg-max exchange of the camera-sharded decision (the reference takes torch.max over all cameras on one GPU,
 * macarons/testers/shapenet.py:172; ties -> first = lowest camera index):
 * mcr_best_record: records[b] = (max_c gains[b,c], idx_offset + argmax) as two fp32 (indices < 2^24 are exact) -- the 8-byte
 *   per-cloud record each rank contributes to one all-gather;
 * mcr_best_merge: records [world,B,2] -> vals[b], idx[b] (int64) of the global maximum. */
int mcr_best_record(const float* gains, int64_t B, int64_t C, int64_t idx_offset, float* records, void* stream);
int mcr_best_merge(const float* records, int world, int64_t B, float* vals, int64_t* idx, void* stream);

/* MACARONS per-camera scoring (predict_coverage_gain_for_single_camera, macarons/utility/macarons_utils.py:1580-1738):
 * mcr_fov_mask_occ: occ_out[c,p] = mask[c,p] ? occ[p] : 0  (frustum mask AND'ed into the sampler's occupancy, :1603-1613)
 * mcr_transform_points: in place pts[i,:3] = (([x y z 1] M_view)[:3] - center) * inv_diag   (:1641-1660)
 * mcr_macarons_gain: vis[b,n] *= factor(d = |pts_world[b,n]-cam_world[b]|), gains[b] = mean_n vis[b,n] * volume[b] (:1699-1704);
 *   factor_mode 0: min(1, (th/d)^2) = get_distance_factor_threshold (:1768-1776) and, with th = focal * epsilon / pixel_size,
 *   get_distance_factor (:1741-1765); factor_mode 1: 1 / (1 + (d/th)^2) = get_distance_factor_smooth (:1779-1788). */
int mcr_fov_mask_occ(const unsigned char* mask, const float* occ, int64_t occ_stride, float* occ_out, int64_t P, int n_cam,
                     void* stream);
int mcr_transform_points(float* pts, int pts_dim, int64_t n, const float* M_view, const float* center, float inv_diag,
                         void* stream);
/* All clouds in one launch: cloud c (pts_per_cloud consecutive rows, or, with cloud_of != NULL, the n_points rows whose
 * cloud_of[i] == c -- ragged clouds) uses M_view[c] (16 floats), center[c] (3 floats) and inv_diag[c]: the K neighbour cameras'
 * sampled sets, or the per-cell clouds of the occupancy-field pass, go to their prediction spaces together. */
int mcr_transform_points_batched(float* pts, int pts_dim, int64_t n_clouds, int64_t pts_per_cloud, const float* M_view,
                                 const float* center, const float* inv_diag, const int* cloud_of, int64_t n_points, void* stream);
int mcr_macarons_gain(float* vis, const float* pts_world, int pts_dim, const float* cam_world, const float* volume,
                      float distance_th, int factor_mode, int64_t B, int64_t N, float* gains, void* stream);

/* ---- scene-side point bookkeeping ---------------------------------------------------------
 * mcr_min_dist_segmented (K11): dmin[i] = min_j |A[i] - B[j]| in fp64 over the B points of A[i]'s segment (grid cell);
 *   replaces torch.min(torch.cdist(a.double(), b.double())) of Cell.fill / camera_coverage_gain / scene_coverage
 *   (macarons/utility/macarons_utils.py:2566, :3022, :3049).  Offsets are CSR int64 [n_segments+1]; +inf if B is empty.
 * mcr_unproject_depth (K12): Camera.project_depth_in_3D / utils.project_depth_back_to_3D (macarons_utils.py:2339-2360,
 *   utils.py:1458-1487): depth [n_cam,H,W] -> world [n_cam,H*W,3]; each camera = 18 floats: inverse full projection
 *   matrix (row-major, row-vector convention) + k22, k32 of the projection matrix (scaled-depth conversion). */
/* mcr_signed_distance_to_depth: Camera.get_signed_distance_to_depth_maps (macarons_utils.py:2451-2500) for one camera / depth
 *   map: sgn[i] = z_view(pts[i]) - bilinear(depth)(projection of pts[i]), grid_sample(bilinear, border, align_corners=False)
 *   semantics; camera = 32 floats M_view[16] | M_full_projection[16] (row-major, row-vector convention); depth [H,W];
 *   mask [H,W] bytes or NULL: pixels with mask == 0 count as `fill` (the reference writes 1.1 zfar there, :2479).
 * mcr_proxy_scene_update: the proxy-point bookkeeping of one MACARONS step after a new depth map (testers/scene.py:402-418:
 *   signed distances, Scene.update_proxy_view_states :2817-2877, update_proxy_supervision_occ :2888-2912,
 *   update_proxy_out_of_field :2879-2886) fused in one pass over the P proxy points; fov_mask [P] bytes selects the points in
 *   the current frustum (mcr_points_in_fov); X_cam = 3 device floats (the camera centre); per-point state tensors are updated
 *   in place: view_states [P, n_elev*n_azim] (0/1; the bin towards the camera is OR'ed in where the signed distance is below
 *   distance_to_surface), n_inside / n_behind / supervision_occ / out_of_field [P].  sgn [P] (optional) receives the signed
 *   distances of the masked points. */
int mcr_signed_distance_to_depth(const float* pts, int64_t n, const float* camera, const float* depth, const unsigned char* mask,
                                 int H, int W, float fill, float* sgn, void* stream);
int mcr_proxy_scene_update(const float* proxy_points, int64_t P, const unsigned char* fov_mask, const float* camera, const float* depth,
                           const unsigned char* depth_mask, int H, int W, float fill, const float* X_cam, float distance_to_surface,
                           float tol, float score_threshold, int n_elev, int n_azim, float* view_states, float* n_inside,
                           float* n_behind, float* supervision_occ, float* out_of_field, float* sgn, void* stream);
/* The online trainer's K-frame passes over the proxy points (trainers/train_macarons.py:386-415 = :616-661, and :476-487 = :719-730);
 * 1 <= K <= 32 frames, refused otherwise before anything else is looked at.  One thread per proxy point, no atomics.
 * mcr_supervision_frames: cameras [K,40] (mcr_points_in_fov records), depth [K,H,W], depth_mask [K,H,W] bytes or NULL, fill = K HOST
 *   floats (1.1 zfar per frame) -> fov_bits [P] uint32 (bit k = mcr_points_in_fov of camera k), sgn [K,P] (mcr_signed_distance_to_depth
 *   of frame k where bit k is set, 0 elsewhere), close_mask [P] bytes: `close[fov_mask_k] = |sgn_k| < surface_distance` frame after
 *   frame (:415), i.e. the test of the LAST frame whose frustum holds the point, 0 for a point in no frustum.
 * mcr_proxy_scene_update_frames: what K successive mcr_proxy_scene_update calls leave in the five state tensors, from fov_bits and sgn
 *   (the depth maps are not sampled again); X_cam [K,3] device floats. */
int mcr_supervision_frames(const float* proxy_points, int64_t P, const float* cameras, int K, const float* depth,
                           const unsigned char* depth_mask, int H, int W, const float* fill, float surface_distance, uint32_t* fov_bits,
                           float* sgn, unsigned char* close_mask, void* stream);
int mcr_proxy_scene_update_frames(const float* proxy_points, int64_t P, const uint32_t* fov_bits, const float* sgn, int K,
                                  const float* X_cam, float distance_to_surface, float tol, float score_threshold, int n_elev,
                                  int n_azim, float* view_states, float* n_inside, float* n_behind, float* supervision_occ,
                                  float* out_of_field, void* stream);
int mcr_min_dist_segmented(const float* A, const int64_t* a_offsets, const float* B, const int64_t* b_offsets, int64_t n_segments,
                           int64_t max_a_per_segment, double* dmin, void* stream);
int mcr_unproject_depth(const float* depth, int H, int W, const float* cameras, int64_t n_cam, float* world, void* stream);

/* ---- scene-grid bookkeeping fused (Scene.fill_cells macarons_utils.py:2727-2737 over Cell.fill :2551-2577; the cell lookup of
 * compute_scene_occupancy_probability_field :1434) --------------------------------------------------------------------------------
 * mcr_cell_keys: key[i] = linear id ((i_l * grid_w + i_w) * grid_h + i_h) of the cell point i falls in by upstream's floor rule
 *   (utils.floor_divide :113-117 on pts - x_min, capped at grid - 1); box_test != 0: n_cells instead when the point is outside the
 *   scene box [x_min, x_max] (closed, get_pts_in_bounding_box :2676-2691), not STRICTLY inside its cell's box (lo_tab / hi_tab
 *   [n_cells, 3]: Cell.fill's two masks) or not offered (valid[i] == 0; valid may be NULL).  grid_consts = x_min[3] x_max[3] step[3].
 * mcr_key_histogram: counts[k] = #{i: key[i] == k}, k = 0 .. nk, and their exclusive prefix sums offsets[0 .. nk + 1]  (nk <= 1023).
 * mcr_admit_keys: Cell.fill's admission on candidates sorted by cell: key2[i] = key_s[i] if the cell has more than n_point_min
 *   candidates (cand[key]) and the candidate's fp64 distance d[i] to the cell's stored points exceeds `resolution`, else nk. */
int mcr_cell_keys(const float* pts, int64_t N, const unsigned char* valid, const float* grid_consts, int grid_l, int grid_w, int grid_h,
                  const float* lo_tab, const float* hi_tab, int box_test, int* key, void* stream);
int mcr_key_histogram(const int* key, int64_t N, int nk, int64_t* counts, int64_t* offsets, void* stream);
int mcr_admit_keys(const double* d, const int* key_s, const int64_t* cand, int64_t N, double resolution, int64_t n_point_min, int nk,
                   int* key2, void* stream);

/* ---- one MACARONS decision without the host glue (testers/scene.py:391-454; macarons/utility/macarons_utils.py:2727-2737 Scene.fill_cells
 * over :2551-2577 Cell.fill, :1395-1540 compute_scene_occupancy_probability_field, :1631-1704 predict_coverage_gain_for_single_camera):
 * each phase of the loop body is a handful of launches behind ONE call, the host reads two small count tables back.
 *
 * mcr_group_by_key: stable grouping of N rows by key[i] in 0 .. nk (anything else counts as nk; nk <= 1023): order[pos] = source row --
 *   rows of one key contiguous, ascending row index inside a key, i.e. torch.sort(key, stable=True).indices -- with counts[0 .. nk] and
 *   their exclusive offsets[0 .. nk + 1].  (The reference compacts with boolean masks cell by cell; the sort replaced it in round 3.)
 *
 * mcr_scene_fill_begin: the device part of Scene.fill_cells for ALL cells: key[i] = cell of point i (mcr_cell_keys, box_test = 1),
 *   order = candidates grouped by cell, dmin[i] = fp64 distance of the i-th candidate IN CELL ORDER to the store of its cell
 *   (store_pts: every cell's stored points, cells in linear order; store_off [n_cells + 1] their offsets), key2 / order2 = the admitted
 *   candidates (Cell.fill :2562-2568) grouped by cell.  counts [4 n_cells + 7] = cand [n_cells+1] | a_off [n_cells+2] | adm [n_cells+1] |
 *   adm_off [n_cells+2] | n_ambiguous [1]: the number of offered in-box points that a cell OTHER than their floor cell strictly contains
 *   (written by every call, 0 = none).  Upstream offers every in-box point to every englobing cell; for such a point the floor rule and
 *   upstream's may part, and the caller fills upstream's way instead (Scene.fill_cells).
 * mcr_scene_fill_gather: new store row r = row g[r] of the virtual table [old store (n_store rows) | admitted candidates in cell order]
 *   (the host builds g from the cells' torch.randperm draws, :2573); features ride along (F floats per row; NULL = none).
 *
 * mcr_field_select: which proxy points take part in the occupancy pass and where (:1428-1442): stored_cell[p] = cell whose store holds
 *   proxy point p (features column 0 = proxy index; `pend_*` = the arrays of a mcr_scene_fill_begin whose gather has not run yet, NULL =
 *   none), proxy_proba <- 0 where seen (:1431), visit[c] = 1 for cells holding a seen point (:1434), rows_order = selected points
 *   grouped by storing cell (ascending index), oof_order = never-seen points first (ascending index).
 *   counts = visit [n+1] | sel_counts [n+1] | sel_off [n+2] | oof_counts [2] | oof_off [3], n = n_cells.
 * mcr_field_build: the (cell, chunk) jobs of the pass from host tables -- jobs [J][4] int64 = first position in rows_order, first query row,
 *   first cloud row, unused; segs [n_seg][4] int64 = first row in S_all (the surface store), first cloud row, job, unused; job_xf [J][20] =
 *   world->view matrix (16, row-vector), box centre in view space (3), 1 / (neighbourhood size x cell diagonal) (:1468-1478) --:
 *   rows [T], row_job [T], X_world [T,3] = the selected proxy points, X_q [T,3] / pc_all [tot,3] = queries / surface clouds in their
 *   jobs' prediction spaces (:1479-1484), vh [T,64] = view harmonics of the rows (mcr_view_harmonics_rows).
 * mcr_view_harmonics_rows: vh[t, k] = sum_v view_states[rows[t], bin_perm[v]] * vh_matrix_t[v, k]: move_view_state_to_view_space
 *   (scone_utils.py:863-931) + compute_view_harmonics (:934-960) of selected rows (rows / bin_perm may be NULL = identity).
 * mcr_field_finish: proxy_proba[rows[t]] = occ[t] (:1525), then the field's tail: the n_oof never-seen points with their stored
 *   probability (:1531-1537).
 *
 * mcr_camera_boxes: per neighbour camera k, centre of the bounding box of its first n_unique[k] sampled points (sampled [K,S,4]) in
 *   the prediction camera's view space (:1631-1641) and the camera centre in the normalised prediction space (:1655-1659).
 * mcr_macarons_gain_indexed: gains[k] = mean_s vis_unique[k, inverse[k,s]] * factor(|world_unique[k, inverse[k,s]] - cam_world[k]|)
 *   * volume[k], 0 when n_unique[k] == 0 (:1668-1704; the Monte-Carlo duplicates read through the inverse map).
 * mcr_philox_uniform_rows: out [K,S] = what K consecutive torch.rand(S, 1, device=...) calls return for a device generator at
 *   (seed, offset): the per-camera sampling uniforms of scone_utils.py:1052 in one launch (mapping 1 = rocRAND's (0,1] map, 0 = cuRAND's). */
size_t mcr_group_by_key_workspace_bytes(int64_t N, int nk);
int mcr_group_by_key(const int* key, int64_t N, int nk, int* order, int64_t* counts, int64_t* offsets, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t mcr_scene_fill_workspace_bytes(int64_t N, int n_cells);
int mcr_scene_fill_begin(const float* pts, int64_t N, const unsigned char* valid, const float* grid_consts, int grid_l, int grid_w,
                         int grid_h, const float* lo_tab, const float* hi_tab, const float* store_pts, const int64_t* store_off,
                         double resolution, int64_t n_point_min, int* key, int* order, double* dmin, int* key2, int* order2,
                         int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int mcr_scene_fill_gather(const int64_t* g, int64_t n_new, const float* store_pts, const float* store_fts, int64_t n_store, int F,
                          const float* pts, const float* features, const int* order, const int* order2, float* new_pts, float* new_fts,
                          void* stream);
/* The same with the row map evaluated on the device: pm = the touched cells' torch.randperm prefixes back to back (int32), tables =
 * new_off | b_off | adm_off | pm_off | touched, int64, n_cells + 1 entries each (offsets of the new store, of the old store, of the
 * admitted candidates, of pm; touched[c] != 0: cell c drew a permutation, else it keeps its rows in order). */
int mcr_scene_fill_gather_perm(const int* pm, const int64_t* tables, int n_cells, int64_t n_new, const float* store_pts,
                               const float* store_fts, int64_t n_store, int F, const float* pts, const float* features, const int* order,
                               const int* order2, float* new_pts, float* new_fts, void* stream);
size_t mcr_field_select_workspace_bytes(int64_t P, int n_cells);
int mcr_field_select(const float* proxy_points, int64_t P, const float* supervision_occ, const float* out_of_field, float* proxy_proba,
                     const float* store_fts, int F, int64_t n_store, const int64_t* store_off, const float* pend_features,
                     const int* pend_order, const int* pend_order2, const int* pend_key2, const int64_t* pend_adm_off, int64_t pend_N,
                     const float* grid_consts, int grid_l, int grid_w, int grid_h, int use_supervision_occ_mask, int* stored_cell,
                     int* key_sel, int* key_oof, int* rows_order, int* oof_order, int64_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);
int mcr_field_build(const int64_t* jobs, int J, const int64_t* segs, int n_seg, const float* job_xf, const int* rows_order,
                    const float* proxy_points, const float* S_all, const float* view_states, int n_bins, const int* bin_perm,
                    const float* vh_matrix_t, int64_t T, int64_t tot, int* rows, int* row_job, float* X_world, float* X_q, float* vh,
                    float* pc_all, void* stream);
int mcr_view_harmonics_rows(const float* view_states, int n_bins, const int* rows, const int* bin_perm, const float* vh_matrix_t,
                            int64_t T, float* vh, void* stream);
int mcr_field_finish(const int* rows, const float* occ, int64_t T, float* proxy_proba, const int* oof_order, int64_t n_oof,
                     const float* proxy_points, float* X_tail, float* occ_tail, void* stream);
int mcr_camera_boxes(const float* sampled, const int* n_unique, int64_t K, int S, const float* M_view, const float* cam_world,
                     float inv_diag, float* center, float* cam_view, void* stream);
int mcr_macarons_gain_indexed(const float* vis_unique, const float* world_unique, const int64_t* inverse, const int* n_unique,
                              const float* cam_world, const float* volume, float distance_th, int factor_mode, int64_t K, int S,
                              float* gains, void* stream);
/* mcr_macarons_gain_backward: gradients of mcr_macarons_gain_indexed for an incoming grad_gains [K] (train_macarons.py:438-444 -> :1259):
 *   d_vis [K,S]: d_vis[k,u] = (grad_gains[k] * volume[k] / S) * #{s : inverse[k,s] == u} * factor(|world[k,u] - cam_world[k]|); rows
 *   u >= n_unique[k] and every row of a camera with n_unique[k] == 0 are exactly 0;  d_volume [K] (NULL: skipped) = grad_gains[k] * the
 *   forward's mean of camera k (accumulated as the forward accumulates it), 0 when n_unique[k] == 0.  world rows have pts_dim >= 3 floats.
 *   inverse == NULL and n_unique == NULL: the identity map, every camera non-empty -- the backward of mcr_macarons_gain (vis = its
 *   input before the in-place scaling).  The counts are an integer LDS histogram (no floating-point atomics: bit-reproducible), which
 *   limits S to 8192; an inverse entry outside [0, S) is skipped. */
int mcr_macarons_gain_backward(const float* grad_gains, const float* vis, const float* world, int pts_dim,
                               const int64_t* inverse /*NULL: identity*/, const int* n_unique /*NULL: all non-empty*/,
                               const float* cam_world, const float* volume, float distance_th, int factor_mode,
                               int64_t K, int S, float* d_vis, float* d_volume /*NULL: skip*/, void* stream);
int mcr_philox_uniform_rows(uint64_t seed, uint64_t offset, int64_t K, int S, int mapping, float* out, void* stream);

/* ---- the occupancy supervision pass of the online trainer (macarons/utility/macarons_utils.py:1233-1392
 * compute_occupancy_probability_for_supervision): selection of the supervised rows and the scatter into upstream's return value.
 *
 * mcr_supervision_select: prediction_mask [P] uint8 = the sampled proxy points (:1260-1278).  englobing[c] = 1 when a sampled point falls
 *   in cell c by the floor rule (:1297, the lookup of mcr_cell_keys with box_test = 0); rows_order = for every cell in linear order the
 *   sampled indices found in that cell's store (store_fts column 0, F floats per row, store_off [n+1]; :1325-1328), ascending, each once
 *   per cell -- an index stored in two cells appears in both; rows_order holds rows_capacity >= n_store entries;
 *   counts = englobing [n+1] | sel_counts [n+1] | sel_off [n+2] | n_pred [1], n = n_cells <= 1023 (entry n of the first two is 0,
 *   sel_off[n] = sel_off[n+1] = the total); pos [P] = rank of p among the set entries of prediction_mask, -1 elsewhere.  rows_order and
 *   sel_off are what mcr_field_build reads as rows_order and "first position in rows_order".  workspace: a bitmap of n x ceil(P/32) words
 *   (integer atomicOr only).
 * mcr_supervision_scatter: out[pos[rows[t]]] += occ[t] from zeros over the rows of the first J jobs (job_offsets [J+1]: job j owns rows
 *   job_offsets[j] .. job_offsets[j+1]-1, ascending indices inside a job), summed in job order (:1371 cell after cell); out [n_out] is
 *   written in every row that pos names.  No floating-point atomics: the bits do not depend on the number of contributions.
 * mcr_supervision_scatter_backward: d_occ[t] = d_out[pos[rows[t]]] for t < T_scatter, 0 for T_scatter <= t < T. */
size_t mcr_supervision_select_workspace_bytes(int64_t P, int n_cells);
int mcr_supervision_select(const unsigned char* prediction_mask, const float* proxy_points, int64_t P, const float* grid_consts, int grid_l,
                           int grid_w, int grid_h, const float* store_fts, int F, int64_t n_store, const int64_t* store_off, int* rows_order,
                           int64_t rows_capacity, int64_t* counts, int* pos, void* workspace, size_t workspace_bytes, void* stream);
int mcr_supervision_scatter(const int* rows, const float* occ, const int64_t* job_offsets, int J, const int* pos, int64_t P, float* out,
                            int64_t n_out, void* stream);
int mcr_supervision_scatter_backward(const int* rows, const int* pos, int64_t P, const float* d_out, int64_t n_out, int64_t T_scatter,
                                     int64_t T, float* d_occ, void* stream);

/* ---- the plane sweep of the depth module (macarons/networks/ManyDepth.py:207-305 CostVolumeBuilder.forward, up to and without the
 * torch.cat / conv_reduce at :299-300), fused (cost_volume.hip).
 *
 * mcr_cost_volume: out[b, k, i, j] = (1/C) sum_c | mean_a warped[b, k, a, c, i, j] - x[b, c, i, j] |, replacing: the B*D and B*D*A
 *   FoVPerspectiveCameras (:233-254), reproject_depth_map of D constant depth maps (:257-261 -> :111-144, unproject_points with
 *   scaled_depth_input=False), warp (:264-282 -> :146-205: transform_points(eps=1e-8) of the full projection transform, the
 *   -min(w,h)/w, -min(w,h)/h factors, F.interpolate(mode='bicubic') of the H x W coordinate images to Hf x Wf, F.grid_sample(bilinear,
 *   zeros, align_corners=False) of D contiguous copies of the source maps), torch.mean over the sources (:288) and the L1 norm over the
 *   channels / C (:291-297).
 *   x [B,C,Hf,Wf] target features, x_alpha [B,A,C,Hf,Wf] source features, depth_bins [D], cams [B,1+A,12]: row 0 the target camera, rows
 *   1..A the sources, each PyTorch3D's R (9 floats, row-major, row-vector convention view = world @ R + T) then T (3 floats).  H x W is
 *   the image size whose pixel grid is unprojected, Hf <= H, Wf <= W, H, W >= 2.  fov_scale = 1 / tan(fov / 2) (upstream: fov = 60
 *   degrees; znear and zfar drop out).  out: batch b starts at out + b * out_batch_stride floats and holds [D,Hf,Wf] contiguous, so out
 *   may be channel C of a [B,C+D,Hf,Wf] buffer (out_batch_stride = (C+D)*Hf*Wf): upstream's cat.  C must be 64.  A resized coordinate that
 *   is not finite or lies a pixel or more outside the source map contributes zero and indexes nothing.  No atomics, fixed summation order:
 *   bit-reproducible.  workspace (16-byte aligned): a channels-last copy of x_alpha. */
size_t mcr_cost_volume_workspace_bytes(int64_t B, int64_t A, int64_t C, int64_t Hf, int64_t Wf);
int mcr_cost_volume(const float* x, const float* x_alpha, const float* cams, const float* depth_bins, float* out,
                    int64_t out_batch_stride, int64_t B, int A, int C, int H, int W, int Hf, int Wf, int D, float fov_scale,
                    void* workspace, size_t workspace_bytes, void* stream);

/* mcr_cost_volume_backward (cost_volume_bwd.hip): the gradients of mcr_cost_volume's x and x_alpha for d_out = d loss / d out; the cameras
 *   and the bins are constants.  With m_c = mean over the sources of the warped channel c and s_c = sign(m_c - x_c), one of -1, 0, +1
 *   (0 where the difference is exactly 0, as torch's abs backward has it: ReLU'd features meet there):
 *     d_x[b,c,p]           = -(1/C)  sum_k d_out[b,k,p] s_c(k,p)
 *     d_x_alpha[b,a,c,y,x] = 1/(A C) sum over the (k, p, corner) whose bilinear corner is pixel (y,x) of  w_corner d_out[b,k,p] s_c(k,p)
 *   x, x_alpha, cams, depth_bins, the sizes and fov_scale as in mcr_cost_volume; the coordinates are computed by the forward's own code.
 *   d_out: batch b starts at d_out + b * d_out_batch_stride floats and holds [D,Hf,Wf] contiguous (channels C.. of the gradient of a
 *   [B,C+D,Hf,Wf] buffer: d_out_batch_stride = (C+D)*Hf*Wf).  d_x [B,C,Hf,Wf] or NULL, d_x_alpha [B,A,C,Hf,Wf] or NULL: a NULL output is
 *   not computed, and its passes do not run (d_x_alpha is the expensive half); both NULL is refused.  A sample that the forward's inside
 *   test rejects has weight 0 here too.  The refusals of mcr_cost_volume, and one more: 4*B*A*D*Hf*Wf (the corner contributions) must not
 *   exceed 2^31 - 1.  No floating-point atomics: d_x sums the planes in ascending order; d_x_alpha is summed per destination pixel from an
 *   inverted index (integer atomics count and place the entries) in 64-bit fixed point, q = llrint(w d_out 2^32 / max|d_out|) per entry,
 *   which no order of the entries changes -- two calls give the same bits.  max|d_out| = 0 gives zero gradients; a d_out with a NaN or an
 *   infinity gives gradients of NaN throughout.  workspace (16-byte aligned): the channels-last copy of x_alpha (reused for its gradient),
 *   the sign states (16 bytes per (b,k,p): nothing here has a channel axis per source, plane and position), the sampled coordinate of every
 *   (b,a,k,p) and the index (8 bytes per corner contribution); mcr_cost_volume_backward_workspace_bytes is 0 for sizes that are not
 *   positive or that the entry refuses. */
size_t mcr_cost_volume_backward_workspace_bytes(int64_t B, int64_t A, int64_t C, int64_t Hf, int64_t Wf, int64_t D);
int mcr_cost_volume_backward(const float* x, const float* x_alpha, const float* cams, const float* depth_bins, const float* d_out,
                             int64_t d_out_batch_stride, float* d_x, float* d_x_alpha, int64_t B, int A, int C, int H, int W, int Hf, int Wf,
                             int D, float fov_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the photometric reconstruction loss of the depth module (macarons/utility/macarons_utils.py:1091-1187 get_reconstruction_loss_fn,
 * with reproject_depth_map / warp of macarons/networks/ManyDepth.py:111-205 and SSIM of :809-842), fused (reconstruction_loss.hip).
 *
 * mcr_reconstruction_loss: loss[s] of S depth maps in one call, replacing per scale: the unprojection and projection, F.grid_sample, the
 *   transpositions, the five average pools over reflection-padded copies, the elementwise chain, the min over the sources and the
 *   masked sum.  images [B,H,W,3], alpha_images [B,A,H,W,3], mask [B,H,W] bytes (non-zero = inside) or NULL, cams [B,1+A,12] as for
 *   mcr_cost_volume, depth [S,B,H,W].  Per pixel (p,q): d = mask ? depth : zfar (a masked-out pixel still warps, at zfar, and still
 *   feeds its neighbours' windows); ray per unit depth ((W/m - 2q/(m-1))/fov_scale, (H/m - 2p/(m-1))/fov_scale, 1), m = min(H,W);
 *   source-view point v, w = sign(v_z) max(|v_z|, 1e-8), grid (-(m/W) fov_scale v_x/w, -(m/H) fov_scale v_y/w); bilinear sample,
 *   align_corners = False, padding_mode 0 = zeros or 1 = border; l1_a = mean_c |I - Iw_a|; ssim_a = mean_c clamp((1 - n/d)/2, 0, 1)
 *   over 3x3 windows of the reflection-padded images (C1 = 1e-4, C2 = 9e-4), the window statistics computed centred on the window's
 *   means; loss_a = ssim_factor ssim_a + (1 - ssim_factor) l1_a (ssim_factor = 0 skips the SSIM part); the min over a, the lowest index
 *   on a tie.  With a mask loss[s] = sum_b sum_p sel mask / (sum_p mask + 1e-7) -- the per-image means SUMMED over the batch, as
 *   upstream has it -- and without one the mean over B H W.  loss_map [S,B,H,W] (the selected loss of every pixel) and argmin
 *   [S,B,H,W] bytes (its source) are written when not NULL.  The pixel coordinate is computed in double (an fp32 coordinate near 456
 *   is spaced 3e-5 apart, which the SSIM gradient magnifies to 1e-3), the samples and the loss in fp32.  A pixel coordinate that is not
 *   finite AS AN FP32 VALUE samples nothing in either padding mode (value 0, no address formed from it; torch leaves the clamp of a NaN
 *   unspecified) -- a finite grid coordinate whose pixel coordinate overflows fp32 included.  Refused before any launch: A outside
 *   1..8, H or W below 2, another padding mode, a workspace that is short or not 16-byte aligned, sizes whose products overflow an
 *   index (S, B <= 65535).  No floating-point atomics: every workgroup stores one partial, a second launch of one workgroup adds them
 *   in a fixed order.  workspace: the partials.
 * mcr_reconstruction_loss_backward: d_depth [S,B,H,W] = d (sum_s d_loss[s] loss[s]) / d depth; images, cameras and mask are constants.
 *   A gather per pixel that recomputes coordinates, samples and selection with the forward's device code (the same bits), no atomics:
 *   two calls give the same bits.  A masked-out pixel's d_depth is exactly 0; the gradient of |x - y| at 0 is 0; a coordinate held by
 *   border's clamp, and the w held by the 1e-8 clamp, pass no gradient.  Same refusals.  workspace: the mask counts of every image.
 * The size functions return 0 for sizes that the entries refuse. */
size_t mcr_reconstruction_loss_workspace_bytes(int64_t S, int64_t B, int64_t A, int64_t H, int64_t W);
int mcr_reconstruction_loss(const float* images, const float* alpha_images, const unsigned char* mask, const float* cams,
                            const float* depth, float* loss, float* loss_map, unsigned char* argmin, int64_t S, int64_t B, int A, int H,
                            int W, float fov_scale, float zfar, float ssim_factor, int padding_mode, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t mcr_reconstruction_loss_backward_workspace_bytes(int64_t S, int64_t B, int64_t A, int64_t H, int64_t W);
int mcr_reconstruction_loss_backward(const float* images, const float* alpha_images, const unsigned char* mask, const float* cams,
                                     const float* depth, const float* d_loss, float* d_depth, int64_t S, int64_t B, int A, int H, int W,
                                     float fov_scale, float zfar, float ssim_factor, int padding_mode, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---- between the depth network's disparity maps and its losses (macarons/utility/macarons_utils.py:959-1031 apply_depth_model, with
 * get_regularity_loss_fn / regularity_tab of depth_model_utils.py:522-562), fused (disparity_scales.hip).
 *
 * mcr_disparity_scales: the depth of S disparity maps at full resolution, their S edge-aware regularity values and the error mask of scale
 *   0 in one call, replacing the S disparity-to-depth conversions, the nearest upsamplings, the depth-to-disparity round trips, the
 *   per-image mean normalisations, the mask zeroings, the S regularity losses and the table of the error mask with its threshold.
 *   disps: a HOST array of S device pointers, disps[s] [B,Hs[s],Ws[s]]; Hs, Ws: HOST arrays of S ints with H = r_s Hs[s] and
 *   W = r_s Ws[s], r_s one of 1, 2, 4, 8, 16 and the same on both axes (for these ratios torch's `nearest` reads source pixel dst / r_s);
 *   all three arrays are read before the entry returns.  images [B,H,W,3], mask [B,H,W] bytes (non-zero = inside) or NULL (nothing is
 *   zeroed).  With a = 1/znear - 1/zfar and b = 1/zfar, per scale, image and full-resolution pixel p = (y,x):
 *     depth[s,b,p] = 1 / (a disp_s[b, y / r_s, x / r_s] + b), [S,B,H,W] as mcr_reconstruction_loss reads it;
 *     D = disp_s[b, y / r_s, x / r_s] -- the entry READS THE DISPARITY DIRECTLY where upstream recomputes it from the depth as
 *       (1/depth - b)/a (the identity to 6e-8 in fp32, derivative 1), so the pixels of an upsampled block compare exactly equal;
 *     n = D / (mu + 1e-7), mu the mean of D over the image, and n = 0 where the mask is zero, BY SELECTION where upstream multiplies by 0:
 *       the two differ only for a disparity that is not finite (0 here, NaN upstream);
 *     reg[s] = mean over B H (W-1) of |n[y,x] - n[y,x+1]| exp(-mean_c |I[y,x] - I[y,x+1]|) + mean over B (H-1) W of the same downwards:
 *       the raw value, the scale weights (1, 1/2, 1/4, 1/8) and params.regularity_factor stay with the caller.
 *   From scale 0 alone, with P(i,j) = n[reflect(i-1), reflect(j-1)] and I_P the image likewise (upstream's table on reflection-padded
 *   copies, with its one-pixel shift up and left): tab[i,j] = |P(i,j) - P(i,j+1)| exp(-mean_c |I_P(i,j) - I_P(i,j+1)|) + the same
 *   downwards; thr[b] = mean(tab_b) + std(tab_b), the std unbiased (N - 1); error_mask [B,H,W] bytes = tab < thr.  The mean and the
 *   variance are formed from per-tile sums of t and of t^2 held and added in double (the square of an fp32 value is exact in double),
 *   never from an fp32 E[t^2] - mean^2.  tab [B,H,W] and thr [B] are written when not NULL.  Refused before any launch: S outside 1..8,
 *   H or W below 2, a scale whose ratio is not in the set or differs between the axes (Hs[s] r_s != H or Ws[s] r_s != W), znear or zfar
 *   not positive and finite, a workspace that is short or not 16-byte aligned, sizes whose products overflow an index (B <= 65535).
 *   Four launches (the S B sums at each scale's own resolution; one 16 x 16 tile of one image for all scales per workgroup; one
 *   workgroup that adds the partials in a fixed order; tab < thr), no floating-point atomics: two calls give the same bits.
 *   workspace: the partials, and the table and thresholds when the caller does not take them.
 * mcr_disparity_scales_backward: d_disps[s] [B,Hs[s],Ws[s]] (a HOST array of S device pointers) = d (sum_p d_depth . depth + sum_s
 *   d_reg[s] reg[s]) / d disp_s, each at its own resolution; images and mask are constants, the error mask has no gradient.
 *   d_depth [S,B,H,W] or NULL, d_reg [S] or NULL: a NULL half is not computed (without d_reg: one launch), both NULL is refused.  With
 *   G[p] = d_reg[s] d reg[s] / d n[p] and m the mask,
 *     d_disp_s[j] = sum over the pixels p of block j of (-a depth[p]^2 d_depth[s,b,p] + m[p] G[p] / (mu + eps))
 *                   - sum over the image of m[p] G[p] D[p] / ((mu + eps)^2 Hs Ws)        (the derivative through the mean: every pixel
 *   of the image receives it, the masked-out ones too, as in upstream where the mean is taken before the mask).  The gradient of |x| at 0
 *   is 0, so the interior of an upsampled block contributes nothing, as in torch; a masked-out pixel's own term is exactly 0.  n is
 *   formed by the forward's device code from the same sums: both directions see the same signs.  Same refusals.  No floating-point
 *   atomics, every sum in a fixed order (a block is summed row by row; 16 is a multiple of every ratio, so no block straddles a tile): two
 *   calls give the same bits.  workspace: the partials.
 * The size functions return 0 for sizes that the entries refuse. */
size_t mcr_disparity_scales_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t W);
int mcr_disparity_scales(const float* const* disps, const int* Hs, const int* Ws, const float* images, const unsigned char* mask,
                         float* depth, float* reg, unsigned char* error_mask, float* tab, float* thr, int S, int64_t B, int H, int W,
                         float znear, float zfar, void* workspace, size_t workspace_bytes, void* stream);
size_t mcr_disparity_scales_backward_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t W);
int mcr_disparity_scales_backward(const float* const* disps, const int* Hs, const int* Ws, const float* images, const unsigned char* mask,
                                  const float* d_depth, const float* d_reg, float* const* d_disps, int S, int64_t B, int H, int W,
                                  float znear, float zfar, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the disparity heads of the depth decoder (macarons/networks/ManyDepth.py:366-384 DisparityLayer, disp1..disp4 of :442-472): a
 * reflection pad, a 3x3 convolution to one output channel and a sigmoid, fused (disparity_head.hip).
 *
 * mcr_disparity_head: x [B,C,Hs,Ws], weight [C,3,3] (upstream's conv.weight [1,C,3,3]), bias [1] -> y [B,Hs,Ws], all contiguous fp32:
 *     z[b,i,j] = bias + sum_c sum_{di,dj in -1..1} weight[c,di+1,dj+1] x[b,c,r(i+di,Hs),r(j+dj,Ws)],   y = 1 / (1 + exp(-z)),
 *   r torch's `reflect` for padding 1 (-1 -> 1, n -> n-2), an index computation: no padded copy exists.  z [B,Hs,Ws], the
 *   pre-activation, is written when not NULL.  One launch: a workgroup owns a tile of one image for all channels (32 x 8 pixels, or 16 x 4
 *   where that would leave compute units idle), stages the tile and its one-pixel ring in LDS 8 (or 24) channels at a time -- every feature is
 *   read from memory once, apart from the ring, along W -- and adds the products in a fixed order (c ascending, the taps row-major, from
 *   the bias): two calls give the same bits.  The weights are read wave-uniformly (scalar loads), never per thread.
 * mcr_disparity_head_backward: with g = d_y y (1 - y) -- y [B,Hs,Ws] is an input, what the forward returned -- and d_y [B,Hs,Ws],
 *     d_bias [1] = sum g;   d_weight [C,3,3]: d_weight[c,t] = sum_{b,i,j} g[b,i,j] x[b,c,r(i+di),r(j+dj)];
 *     d_x [B,C,Hs,Ws]: d_x[b,c,i,j] = the sum of weight[c,t] g[b,q] over every (output pixel q, tap t) whose reflected source is (i,j):
 *   row 1 also receives what padded row -1 would, row Hs-2 what padded row Hs would, the columns likewise, both at the corners; on a
 *   two-pixel axis the two mirrors land on different pixels.  A NULL output is not computed (d_x alone: x may be NULL and is not read;
 *   without d_x weight may be NULL), all three NULL is refused.  d_x is a gather (one launch, x not read); d_weight and d_bias take
 *   two launches: every workgroup stores one partial per sum into the workspace, a second launch adds the partials of each output in a
 *   fixed order, in double.  No floating-point atomics: two calls give the same bits.  workspace: the partials.
 * Both refuse before any launch: Hs or Ws below 2, C outside 1..512, B below 1, B C Hs Ws beyond a 32-bit index, and the backward a
 * workspace that is short or not 16-byte aligned.  The size function returns 0 for sizes that the entries refuse. */
int mcr_disparity_head(const float* x, const float* weight, const float* bias, float* y, float* z, int64_t B, int C, int Hs, int Ws,
                       void* stream);
size_t mcr_disparity_head_backward_workspace_bytes(int64_t B, int64_t C, int64_t Hs, int64_t Ws);
int mcr_disparity_head_backward(const float* x, const float* weight, const float* y, const float* d_y, float* d_x, float* d_weight,
                                float* d_bias, int64_t B, int C, int Hs, int Ws, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the expansion layers of the depth decoder (macarons/networks/ManyDepth.py:308-363 ExpansionLayer, expansion5..1 of :428-471): a
 * transposed 3x3 convolution, ELU, a nearest resize, a channel concatenation, a reflection-padded 3x3 convolution and ELU, fused
 * (expansion_layer.hip) -- the forward.
 *
 * mcr_expansion_layer: x [B,Cin,h,w], x_add [B,Cadd,H,W] (NULL with Cadd = 0), up_weight [Cin,Cmid,3,3] and up_bias [Cmid] (upstream's
 *   upconv), i_weight [Cout,Cmid+Cadd,3,3] and i_bias [Cout] (upstream's iconv) -> y [B,Cout,H,W], all contiguous fp32:
 *     u = ELU(conv_transpose2d(x, up_weight, up_bias; stride 1, padding 1))   [B,Cmid,h,w], kept in the workspace
 *     y = ELU(conv2d(reflect_pad1(cat(nearest(u -> (H,W)), x_add)), i_weight, i_bias))
 *   ELU with alpha 1 (expm1f below zero); nearest is torch's mode='nearest': source = min(floor(dst * (float)in / out), in - 1), in float.
 *   Two launches of one kernel on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32): the first reads the transposed convolution
 *   as a zero-padded correlation with the kernel flipped and the channel axes exchanged; the second applies the reflection index, the
 *   nearest-source index and the u / x_add channel boundary while it stages a tile: no resized, concatenated or padded tensor exists.
 *   Both weights are read in upstream's layouts.  A split of the channel sum among the waves of a workgroup is added in the order of the
 *   waves; no atomics: two calls give the same bits.
 * Refused before any launch: H or W below 2, h or w below 1, Cin, Cmid or Cout outside 1..512, Cadd below 0 or Cmid + Cadd above 512,
 * B below 1, a tensor of 2^31 elements or more, a NULL operand (x_add only with Cadd > 0), a workspace that is missing, short or not
 * 16-byte aligned.  The size function returns 0 for sizes that the entry refuses. */
size_t mcr_expansion_layer_workspace_bytes(int64_t B, int64_t Cmid, int64_t h, int64_t w);
int mcr_expansion_layer(const float* x, const float* x_add, const float* up_weight, const float* up_bias, const float* i_weight,
                        const float* i_bias, float* y, int64_t B, int Cin, int Cmid, int Cadd, int Cout, int h, int w, int H, int W,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- the expansion layers, the backward (expansion_layer_bwd.hip).
 *
 * mcr_expansion_layer_backward: x, x_add, up_weight, i_weight as the forward's; u [B,Cmid,h,w], the transposed convolution after its ELU
 *   (the front of the forward's workspace after a call); y [B,Cout,H,W], what the forward returned; d_y [B,Cout,H,W]; all contiguous fp32.
 *   With near() the nearest-source index, refl() the reflection index, c = cat(nearest(u), x_add):
 *     g2 = d_y (y > 0 ? 1 : y + 1);   d_i_bias [Cout] = sum g2;   d_i_weight [Cout,Cmid+Cadd,3,3] = sum_{b,i,j} g2 c[refl(i+di-1),refl(j+dj-1)];
 *     d_c = the transposed reflection-padded convolution of g2 with i_weight;   d_x_add [B,Cadd,H,W] = d_c[:, Cmid:];
 *     d_u[s,t] = the sum of d_c[:, :Cmid] over the pixels (i,j) with near(i) = s, near(j) = t (none where the map shrinks: 0);
 *     g1 = d_u (u > 0 ? 1 : u + 1);   d_up_bias [Cmid] = sum g1;   d_up_weight [Cin,Cmid,3,3] = sum_{b,s,t} x[s,t] g1[s+ki-1,t+kj-1];
 *     d_x [B,Cin,h,w] = the zero-padded correlation of g1 with up_weight.
 *   Any of the six outputs may be NULL and is then not computed; a launch runs only if an output that is asked for depends on it (with
 *   d_i_weight / d_i_bias alone no data gradient is formed; d_x_add alone needs neither d_x's correlation nor the weight pass of the
 *   transposed convolution); all six NULL is refused.  The two data gradients are launches of the forward's kernel (zero padding, no bias,
 *   no ELU), a gather between them folds the ring, sums the nearest ranges and applies ELU'(u); the two weight gradients run on
 *   v_mfma_f32_16x16x4_f32 over the pixels, nine accumulators per 16 x 16 block of channel pairs and a tenth for the bias gradient,
 *   the pixels divided among workgroups by a rule of the shape alone, one partial per output and workgroup in the workspace, added in
 *   a fixed order in double by a finish launch.  No floating-point atomics: two calls give the same bits.  workspace: g2, the
 *   correlation over the padded domain [B,Cmid+Cadd,H+2,W+2], g1 and the partials.
 * Refused before any launch: what the forward refuses (sizes, a tensor of 2^31 elements or more -- here also the padded correlation --,
 * a NULL operand, x_add only with Cadd > 0), d_x_add with Cadd = 0, a workspace that is missing, short or not 16-byte aligned.  The size
 * function returns 0 for sizes that the entry refuses. */
size_t mcr_expansion_layer_backward_workspace_bytes(int64_t B, int64_t Cin, int64_t Cmid, int64_t Cadd, int64_t Cout, int64_t h, int64_t w,
                                                    int64_t H, int64_t W);
int mcr_expansion_layer_backward(const float* x, const float* x_add, const float* up_weight, const float* i_weight, const float* u,
                                 const float* y, const float* d_y, float* d_x, float* d_x_add, float* d_up_weight, float* d_up_bias,
                                 float* d_i_weight, float* d_i_bias, int64_t B, int Cin, int Cmid, int Cadd, int Cout, int h, int w, int H,
                                 int W, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the front of the depth module's ResNet encoder (macarons/networks/ManyDepth.py:33-50 FeatureExtractor, run on the target and on
 * the source images by DepthDecoder.forward, :486-500): the 7x7 / 2 convolution, BatchNorm, ReLU and the 3x3 / 2 max-pool in one launch
 * (resnet_stem.hip), the basic blocks of `layer1` in two launches each (basic_block.hip) -- the forward, for BatchNorm in EVAL mode.
 *
 * An eval-mode BatchNorm is given as torch's four vectors (weight, bias, running_mean, running_var, each [C]) and eps.  In float, per
 * channel:  a = weight * (1.0f / sqrtf(var + eps));  b = fmaf(-mean, a, bias);  BN(z) = fmaf(z, a, b).
 *
 * mcr_resnet_stem: x [N0,Cin,H,W] and x_more [N1,Cin,H,W] (NULL with N1 = 0; x may be NULL with N0 = 0) are the images 0 .. N0-1 and
 *   N0 .. N0+N1-1, weight [Cout,Cin,7,7], bias [Cout] or NULL, all contiguous fp32:
 *     z      = conv2d(image, weight, bias; stride 2, zero padding 3)        [.,Cout,Hc,Wc], Hc = (H-1)/2+1, Wc = (W-1)/2+1
 *     conv1  = max(fmaf(z + bias, a, b), 0)                                  [N0,Cout,Hc,Wc]: for x's images only; may be NULL, then not written
 *     pooled = max_pool2d(., 3, stride 2, padding 1)                         [N0+N1,Cout,Hp,Wp], Hp = (Hc-1)/2+1, Wp = (Wc-1)/2+1;
 *   window cells outside the map are ignored.  One launch on v_mfma_f32_16x16x4_f32 (K = Cin 49 in the weight's order, padded with
 *   zeros to a multiple of 4); a workgroup owns 2 x 15 pooled pixels of an image and every output channel, stages the input tile once
 *   (even and odd columns apart, for the stride) and the weights in LDS, recomputes the one-row, one-column halo of the pooling windows,
 *   and pools out of LDS.  No atomics: two calls give the same bits.
 * mcr_basic_block: x, y [B,C,H,W] (y not x), w1 and w2 [C,C,3,3] (stride 1, zero padding 1, no bias), two BatchNorms:
 *     t = max(BN1(conv2d(x, w1)), 0)   [B,C,H,W], kept at the front of the workspace;     y = max(BN2(conv2d(t, w2)) + x, 0)
 *   Two launches of the expansion layers' kernel with an epilogue of scale, shift, residual and ReLU.
 * mcr_feature_extractor: the stem, then n_blocks (0..4) basic blocks on `pooled` -> features [N0+N1,Cout,Hp,Wp] and, where asked for,
 *   conv1 [N0,Cout,Hc,Wc]: 1 + 2 n_blocks launches.  block_pointers: a HOST array of ten device pointers per block (w1, bn1 weight, bias,
 *   mean, var, w2, bn2 weight, bias, mean, var); block_eps: a HOST array of two eps per block.
 * Refused before any launch: H or W below 1, Cin outside 1..8 and Cout outside 1..64 (the stem), C outside 1..512 (the block), n_blocks
 * outside 0..4, N0 or N1 below 0 or N0 + N1 below 1, B below 1, a tensor of 2^31 elements or more, a NULL operand (x only with N0 > 0,
 * x_more only with N1 > 0; conv1 and the convolution's bias are optional), a workspace that is missing, short or not 16-byte aligned
 * (the block, and the extractor with n_blocks > 0; the stem takes none).  The size functions return 0 for sizes that the entries refuse;
 * the extractor's also for n_blocks = 0, which needs no scratch: its workspace may then be NULL. */
int mcr_resnet_stem(const float* x, const float* x_more, const float* weight, const float* bias, const float* bn_weight,
                    const float* bn_bias, const float* bn_mean, const float* bn_var, float eps, float* pooled, float* conv1, int64_t N0,
                    int64_t N1, int Cin, int Cout, int H, int W, void* stream);
size_t mcr_basic_block_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int mcr_basic_block(const float* x, const float* w1, const float* bn1_weight, const float* bn1_bias, const float* bn1_mean,
                    const float* bn1_var, float eps1, const float* w2, const float* bn2_weight, const float* bn2_bias,
                    const float* bn2_mean, const float* bn2_var, float eps2, float* y, int64_t B, int C, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t mcr_feature_extractor_workspace_bytes(int64_t N0, int64_t N1, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int64_t n_blocks);
int mcr_feature_extractor(const float* x, const float* x_more, const float* weight, const float* bias, const float* bn_weight,
                          const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                          const float* const* block_pointers, const float* block_eps, int n_blocks, float* features, float* conv1,
                          int64_t N0, int64_t N1, int Cin, int Cout, int H, int W, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MACARONS_HIP_H */
