// The forward building blocks (nn_kernels.hip, attention_planes.hip, linear3p.hip), each behind its own C entry point
// (include/macarons_hip.h): used by the host mirrors of Attention.py's modules and by the block-level tests.  The networks call the
// launchers directly; an entry forwards to the same launcher after checking on the host what its kernel assumes.  The TEST entries add no
// kernel.  The backward side is bwd_blocks.hip.
#include "encoder.h"      // (the operand structs, the launchers, Numerics; declares launch_nonfinite_flag, defined here, for scone_occ.hip)
#include <algorithm>

namespace mcr {

__global__ void nonfinite_flag_kernel(const float* __restrict__ x, long long n, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        bad |= !(fabsf(x[i]) <= 3.4028234663852886e38f);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
void launch_nonfinite_flag(hipStream_t s, const float* x, int64_t n, int* flag) {
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 1024)), dim3(256), 0, s, x, (long long)n, flag);
}

// What mcr_attention, _masked, _ws and _lens check alike, in the order they report it.  pointers: the entry's own non-null test; short_ok: the
// call runs the 16-token kernel, which takes any number of sequences; long_limit: the sequences the other kernels take (one grid.z slot each)
static int check_attention(const char* who, bool pointers, int64_t S, int64_t L, bool short_ok, int64_t long_limit, int n_heads, int qk_dim,
                           int v_dim, int64_t ldq, int64_t ldo) {
    MCR_REQUIRE(pointers, "%s: null pointer", who);
    MCR_REQUIRE(S > 0 && L > 0, "%s: empty problem", who);
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "%s: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)", who, n_heads, qk_dim, v_dim);
    MCR_REQUIRE(short_ok || S <= long_limit, "%s: too many long sequences", who);
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "%s: leading dimension too small", who);
    return 0;
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
// the two planes GEMM entries: their operand planes are the sources of 16-byte DMA
static int check_operand_planes(const char* who, const void* Xh, const void* Xl, const void* Wh, const void* Wl, int n_planes) {
    MCR_REQUIRE(al16(Xh) && al16(Wh) && (n_planes == 1 || (al16(Xl) && al16(Wl))), "%s: operand planes must be 16-byte aligned", who);
    return 0;
}

}  // namespace mcr

using namespace mcr;

extern "C" {

int mcr_linear(const float* X, int64_t ldx, const float* W, const float* bias, const float* residual, int64_t ldr, float* Y,
               int64_t ldy, int64_t M, int N, int K, int gelu, void* stream) {
    VariantScope variant_scope_;             // (consumes the thread's one-shot like every scoped entry; the fp32 route reads no variant)
    MCR_REQUIRE(X && W && Y, "mcr_linear: null pointer");
    MCR_REQUIRE(M > 0 && N > 0 && K > 0, "mcr_linear: empty problem");
    MCR_REQUIRE(ldx >= K && ldy >= N && (!residual || ldr >= N), "mcr_linear: leading dimension too small");
    launch_linear((hipStream_t)stream, {X, ldx}, {W, K}, {bias, gelu ? ACT_GELU : ACT_NONE, {residual, ldr}}, {Y, ldy}, M, N, K, /*route_rows=*/0);
    MCR_LAUNCH_CHECK("mcr_linear");
    return 0;
}

int mcr_layernorm(const float* X, int64_t ldx, const float* gamma, const float* beta, float* Y, int64_t ldy, int64_t M, int E,
                  void* stream) {
    MCR_REQUIRE(X && gamma && beta && Y, "mcr_layernorm: null pointer");
    MCR_REQUIRE(M > 0 && E > 0 && E <= 512, "mcr_layernorm: need 0 < E <= 512 (got %d)", E);
    MCR_REQUIRE(ldx >= E && ldy >= E, "mcr_layernorm: leading dimension too small");
    launch_layernorm((hipStream_t)stream, X, ldx, gamma, beta, Y, ldy, M, E);
    MCR_LAUNCH_CHECK("mcr_layernorm");
    return 0;
}

int mcr_attention(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                  int v_dim, void* stream) {
    VariantScope variant_scope_;
    if (check_attention("mcr_attention", qkv && out, S, L, L == 16, 65535, n_heads, qk_dim, v_dim, ldq, ldo)) return 1;
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, nullptr, AttnSplit{},
                     variant_scope_.numerics().attn_pv_half());
    MCR_LAUNCH_CHECK("mcr_attention");
    return 0;
}

int mcr_attention_masked(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                         const unsigned char* mask, int64_t mask_seq_stride, int64_t mask_head_stride, int64_t mask_query_stride,
                         void* workspace, size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    if (check_attention("mcr_attention_masked", qkv && out && mask, S, L, L == 16, 32767, n_heads, qk_dim, v_dim, ldq, ldo)) return 1;
    MCR_REQUIRE(mask_seq_stride >= 0 && mask_head_stride >= 0 && mask_query_stride >= 0, "mcr_attention_masked: negative mask stride");
    const AttnSplit split{(float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, /*mode=*/-1};
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, nullptr, split,
                     AttnMask{mask, mask_seq_stride, mask_head_stride, mask_query_stride});
    MCR_LAUNCH_CHECK("mcr_attention_masked");
    return 0;
}

size_t mcr_attention_workspace_bytes(int64_t S, int64_t L, int n_heads, int v_dim) {
    return attention_split_floats(S, (int)L, n_heads, v_dim) * sizeof(float);
}

int mcr_attention_ws(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim,
                     int v_dim, void* workspace, size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    if (check_attention("mcr_attention_ws", qkv && out, S, L, L == 16, 32767, n_heads, qk_dim, v_dim, ldq, ldo)) return 1;
    const AttnSplit split{(float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, /*mode=*/-1};
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, nullptr, split,
                     variant_scope_.numerics().attn_pv_half());
    MCR_LAUNCH_CHECK("mcr_attention_ws");
    return 0;
}

// TEST entry: launch_attention as the encoders call it (pct.hip: run_encoder*, pct_bwd.hip) -- per-sequence lengths and an explicit
// split mode.
int mcr_attention_lens(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                       const int* lens, int split_mode, void* workspace, size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    // (with lens a 16-token sequence runs the matrix-pipe kernel too: one grid.z slot per sequence)
    if (check_attention("mcr_attention_lens", qkv && out, S, L, L == 16 && !lens, 32767, n_heads, qk_dim, v_dim, ldq, ldo)) return 1;
    MCR_REQUIRE(split_mode >= -1 && split_mode <= 1, "mcr_attention_lens: split_mode must be 1, 0 or -1 (got %d)", split_mode);
    // the launcher drops to the unsplit form when the scratch is short; here a split that was asked for must be possible
    if (split_mode != 0 && L >= 512 && (workspace || split_mode == 1)) {
        MCR_REQUIRE(workspace && workspace_bytes >= mcr_attention_workspace_bytes(S, L, n_heads, v_dim),
                    "mcr_attention_lens: workspace too small for the key split (%zu bytes, %zu needed)", workspace ? workspace_bytes : (size_t)0,
                    mcr_attention_workspace_bytes(S, L, n_heads, v_dim));
        MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "mcr_attention_lens: the workspace must be 16-byte aligned");
    }
    const AttnSplit split{(float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, split_mode};
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, lens, split,
                     variant_scope_.numerics().attn_pv_half());
    MCR_LAUNCH_CHECK("mcr_attention_lens");      // (lens off the matrix-pipe kernel: the launcher's refusal, 3)
    return 0;
}

// planes [2][T][W3] fp16 (the bytes of the fp32 rows) + key-split scratch
struct AttnPlanesScratch { _Float16* planes; float* split; };
static AttnPlanesScratch carve_attention_planes(Arena& a, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim) {
    AttnPlanesScratch w;
    w.planes = reinterpret_cast<_Float16*>(a.f((size_t)S * L * (2 * qk_dim + v_dim)));
    w.split = a.f(attention_split_floats(S, (int)L, n_heads, v_dim));
    return w;
}
size_t mcr_attention_planes_workspace_bytes(int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim) {
    return measure(carve_attention_planes, S, L, n_heads, qk_dim, v_dim);
}

// (no VariantScope: always both planes, whatever the caller's variant.  Its checks stay its own: one size check with its own text and no
// 16-token exemption, the workspace in front of the leading dimensions)
int mcr_attention_planes(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                         const int* lens, int split_mode, void* workspace, size_t workspace_bytes, void* stream) {
    MCR_REQUIRE(qkv && out && workspace, "mcr_attention_planes: null pointer");
    MCR_REQUIRE(S > 0 && L > 0 && S <= 32767, "mcr_attention_planes: bad problem size");
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "mcr_attention_planes: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)",
                n_heads, qk_dim, v_dim);
    MCR_REQUIRE(workspace_bytes >= mcr_attention_planes_workspace_bytes(S, L, n_heads, qk_dim, v_dim), "mcr_attention_planes: workspace too small");
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "mcr_attention_planes: leading dimension too small");
    // the rows are split into planes four floats at a time (split_to_planes_kernel: 16-byte loads), the planes read by 16-byte DMA
    MCR_REQUIRE(ldq % 4 == 0 && ((uintptr_t)qkv | (uintptr_t)workspace) % 16 == 0,
                "mcr_attention_planes: ldq must be a multiple of 4, qkv and workspace 16-byte aligned");
    const int W3 = 2 * qk_dim + v_dim;
    const int64_t T = S * L;
    Arena a{(char*)workspace, workspace_bytes};
    const AttnPlanesScratch ws = carve_attention_planes(a, S, L, n_heads, qk_dim, v_dim);
    MCR_REQUIRE(a.ok(), "mcr_attention_planes: workspace too small");
    const Planes P = planes_over(ws.planes, T, W3);
    launch_split_to_planes((hipStream_t)stream, {qkv, ldq}, P, T, W3);
    launch_attention_planes((hipStream_t)stream, P, {out, ldo}, Planes{}, S, (int)L, n_heads, qk_dim, v_dim, lens,
                            {ws.split, attention_split_floats(S, (int)L, n_heads, v_dim), split_mode}, /*n_planes=*/2);
    MCR_LAUNCH_CHECK("mcr_attention_planes");
    return 0;
}

int mcr_colmax_broadcast(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, void* stream) {
    MCR_REQUIRE(X && Y && S > 0 && L > 0 && E > 0, "mcr_colmax_broadcast: bad arguments");
    MCR_REQUIRE(ldx >= E && ldy >= E, "mcr_colmax_broadcast: leading dimension too small");
    launch_colmax_broadcast((hipStream_t)stream, X, ldx, Y, ldy, S, (int)L, E);
    MCR_LAUNCH_CHECK("mcr_colmax_broadcast");
    return 0;
}

int mcr_pool_max_avg(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, void* stream) {
    MCR_REQUIRE(X && Y && S > 0 && L > 0 && E > 0, "mcr_pool_max_avg: bad arguments");
    MCR_REQUIRE(ldx >= E && ldy >= 2 * (int64_t)E, "mcr_pool_max_avg: leading dimension too small");
    launch_pool_max_avg((hipStream_t)stream, X, ldx, Y, ldy, S, (int)L, E);
    MCR_LAUNCH_CHECK("mcr_pool_max_avg");
    return 0;
}

// TEST entries: the padded-sequence forms of the two launchers above, as run_pct and the SconeVis embedding call them
// (lens: device int [S], may be NULL).
int mcr_pool_max_avg_lens(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, const int* lens, void* stream) {
    MCR_REQUIRE(X && Y && S > 0 && L > 0 && E > 0, "mcr_pool_max_avg_lens: bad arguments");
    MCR_REQUIRE(L <= 0x7fffffffll, "mcr_pool_max_avg_lens: L must fit an int");
    MCR_REQUIRE(ldx >= E && ldy >= 2 * (int64_t)E, "mcr_pool_max_avg_lens: leading dimension too small");
    launch_pool_max_avg((hipStream_t)stream, X, ldx, Y, ldy, S, (int)L, E, lens);
    MCR_LAUNCH_CHECK("mcr_pool_max_avg_lens");
    return 0;
}

int mcr_colmax_broadcast_lens(const float* X, int64_t ldx, float* Y, int64_t ldy, int64_t S, int64_t L, int E, const int* lens, const float* ex,
                              int64_t ex_ld, int ex_cols, float* ex_dst, void* stream) {
    MCR_REQUIRE(X && Y && S > 0 && L > 0 && E > 0, "mcr_colmax_broadcast_lens: bad arguments");
    MCR_REQUIRE(L <= 0x7fffffffll, "mcr_colmax_broadcast_lens: L must fit an int");
    MCR_REQUIRE(ldx >= E && ldy >= E, "mcr_colmax_broadcast_lens: leading dimension too small");
    if (ex) {
        // pool_long_kernel / copy2d_kernel: column j < ex_cols of row m is read at ex[m * ex_ld + j] (ex_ld an int) and written at
        // ex_dst[m * ldy + j]
        MCR_REQUIRE(ex_dst, "mcr_colmax_broadcast_lens: ex without ex_dst");
        MCR_REQUIRE(ex_cols > 0 && ex_cols <= ex_ld && ex_cols <= ldy, "mcr_colmax_broadcast_lens: need 0 < ex_cols <= ex_ld and ex_cols <= ldy (got %d)", ex_cols);
        MCR_REQUIRE(ex_ld <= 0x7fffffffll, "mcr_colmax_broadcast_lens: ex_ld must fit an int");
    } else {
        MCR_REQUIRE(ex_cols == 0 && !ex_dst, "mcr_colmax_broadcast_lens: ex_cols / ex_dst without ex");
    }
    launch_colmax_broadcast((hipStream_t)stream, X, ldx, Y, ldy, S, (int)L, E, lens, ex, (int)ex_ld, ex_cols, ex_dst);
    MCR_LAUNCH_CHECK("mcr_colmax_broadcast_lens");
    return 0;
}

// *flag |= 1 if any of x[0 .. n) is inf / NaN: the range guard of the fp16-split matrix path for outputs that leave through an entry
// point without a flag of its own (SconeVis' harmonics)
int mcr_nonfinite_flag(const float* x, int64_t n, int* flag, void* stream) {
    MCR_REQUIRE(x && flag && n > 0, "mcr_nonfinite_flag: bad arguments");
    launch_nonfinite_flag((hipStream_t)stream, x, n, flag);
    MCR_LAUNCH_CHECK("nonfinite_flag_kernel");
    return 0;
}

// ---- the planes GEMMs of variants 6 / 7 (linear3p.hip) as blocks of their own: bring-up / test entries ----
int mcr_split_to_planes(const float* X, int64_t ldx, void* Ph, void* Pl, int64_t ldp, int64_t M, int E, void* stream) {
    MCR_REQUIRE(X && Ph, "mcr_split_to_planes: null pointer");
    MCR_REQUIRE(M > 0 && E > 0 && E % 4 == 0, "mcr_split_to_planes: need M > 0 and E a positive multiple of 4 (got %d)", E);
    MCR_REQUIRE(ldx >= E && ldp >= E, "mcr_split_to_planes: leading dimension too small");
    // one thread moves four values: a 16-byte load of X, an 8-byte store per plane
    MCR_REQUIRE(ldx % 4 == 0 && al16(X), "mcr_split_to_planes: ldx must be a multiple of 4 and X 16-byte aligned");
    MCR_REQUIRE(ldp % 4 == 0 && al8(Ph) && al8(Pl), "mcr_split_to_planes: ldp must be a multiple of 4 and the planes 8-byte aligned");
    launch_split_to_planes((hipStream_t)stream, {X, ldx}, {(_Float16*)Ph, (_Float16*)Pl, ldp}, M, E);
    MCR_LAUNCH_CHECK("mcr_split_to_planes");
    return 0;
}

// LayerNorm whose rows leave as planes (the encoders' norm1 / norm2 and the PCTransformer's norm on the planes path).  The operands obey
// mcr_split_to_planes' rules, so that the two-step form mcr_split_to_planes(mcr_layernorm(x)) takes the same arguments.
int mcr_layernorm_planes(const float* X, int64_t ldx, const float* gamma, const float* beta, void* Yh, void* Yl, int64_t ldp, int64_t M, int E,
                         void* stream) {
    MCR_REQUIRE(X && gamma && beta && Yh, "mcr_layernorm_planes: null pointer");
    MCR_REQUIRE(M > 0 && E > 0 && E <= 512 && E % 4 == 0, "mcr_layernorm_planes: need M > 0 and E a multiple of 4 in 4 .. 512 (got %d)", E);
    MCR_REQUIRE(ldx >= E && ldp >= E, "mcr_layernorm_planes: leading dimension too small");
    MCR_REQUIRE(ldx % 4 == 0 && al16(X), "mcr_layernorm_planes: ldx must be a multiple of 4 and X 16-byte aligned");
    MCR_REQUIRE(ldp % 4 == 0 && al8(Yh) && al8(Yl), "mcr_layernorm_planes: ldp must be a multiple of 4 and the planes 8-byte aligned");
    launch_layernorm_planes((hipStream_t)stream, {X, ldx}, gamma, beta, {(_Float16*)Yh, (_Float16*)Yl, ldp}, M, E);
    MCR_LAUNCH_CHECK("mcr_layernorm_planes");
    return 0;
}

int mcr_linear_planes(const void* Xh, const void* Xl, int64_t ldx, const void* Wh, const void* Wl, int64_t ldw, const float* bias, float* Y,
                      void* Yh, void* Yl, int64_t ldy, int64_t M, int N, int K, int gelu, float wscale_inv, const float* row_bias,
                      int64_t rows_per_group, const int* row_group, const float* R, int64_t ldr, int n_planes, void* stream) {
    MCR_REQUIRE(n_planes == 1 || n_planes == 2, "mcr_linear_planes: n_planes must be 1 or 2 (got %d)", n_planes);
    MCR_REQUIRE(Xh && Wh && (n_planes == 1 || (Xl && Wl)), "mcr_linear_planes: null operand plane");
    MCR_REQUIRE((Y != nullptr) != (Yh != nullptr), "mcr_linear_planes: exactly one of Y and Yh must be given");
    MCR_REQUIRE(!Yh || n_planes == 1 || Yl, "mcr_linear_planes: null low output plane");
    MCR_REQUIRE(M > 0 && N > 0 && K > 0, "mcr_linear_planes: empty problem");
    MCR_REQUIRE(linear3p_applicable(N, K, ldx, ldw, ldy),
                "mcr_linear_planes: need K a multiple of 32, N a multiple of 4, ldx and ldw multiples of 8, ldy a multiple of 4");
    MCR_REQUIRE(ldx >= K && ldw >= K && ldy >= N && (!R || ldr >= N), "mcr_linear_planes: leading dimension too small");
    if (check_operand_planes("mcr_linear_planes", Xh, Xl, Wh, Wl, n_planes)) return 1;
    // bias rows are read by 16-byte loads at columns that are multiples of 4
    MCR_REQUIRE(al16(bias) && al16(row_bias), "mcr_linear_planes: bias and row_bias must be 16-byte aligned");
    MCR_REQUIRE(!Yh || (al8(Yh) && (n_planes == 1 || al8(Yl))), "mcr_linear_planes: output planes must be 8-byte aligned");
    MCR_REQUIRE(((uintptr_t)Y | (uintptr_t)R) % 4 == 0, "mcr_linear_planes: Y and R must be 4-byte aligned");
    MCR_REQUIRE(!R || Y, "mcr_linear_planes: a residual needs fp32 output");
    MCR_REQUIRE(!row_bias || rows_per_group > 0 || row_group, "mcr_linear_planes: row_bias needs rows_per_group > 0 or row_group");
    const Planes X{(_Float16*)Xh, (_Float16*)Xl, ldx};                  // (read only: the launchers never write their X operand)
    const WPlanes W{(const _Float16*)Wh, (const _Float16*)Wl, ldw, wscale_inv};
    const Epilogue e{bias, gelu ? ACT_GELU : ACT_NONE, {R, ldr}, {row_bias, rows_per_group, row_group}};
    if (Yh) launch_linear3p((hipStream_t)stream, X, W, e, Planes{(_Float16*)Yh, (_Float16*)Yl, ldy}, M, N, K, n_planes);
    else launch_linear3p((hipStream_t)stream, X, W, e, RowsOut{Y, ldy}, M, N, K, n_planes);
    MCR_LAUNCH_CHECK("mcr_linear_planes");
    return 0;
}

int mcr_linear_planes_dot(const void* Xh, const void* Xl, int64_t ldx, const void* Wh, const void* Wl, int64_t ldw, const float* bias, int64_t M,
                          int K, int gelu, float wscale_inv, const float* v, const float* c, int gelu2, float* out, int n_planes, void* stream) {
    MCR_REQUIRE(n_planes == 1 || n_planes == 2, "mcr_linear_planes_dot: n_planes must be 1 or 2 (got %d)", n_planes);
    MCR_REQUIRE(Xh && Wh && (n_planes == 1 || (Xl && Wl)) && v && out, "mcr_linear_planes_dot: null pointer");
    MCR_REQUIRE(M > 0 && K > 0, "mcr_linear_planes_dot: empty problem");
    MCR_REQUIRE(linear3p_applicable(256, K, ldx, ldw, 4), "mcr_linear_planes_dot: need K a multiple of 32, ldx and ldw multiples of 8");
    MCR_REQUIRE(ldx >= K && ldw >= K, "mcr_linear_planes_dot: leading dimension too small");
    if (check_operand_planes("mcr_linear_planes_dot", Xh, Xl, Wh, Wl, n_planes)) return 1;
    MCR_REQUIRE(al16(bias) && al16(v), "mcr_linear_planes_dot: bias and v must be 16-byte aligned");
    MCR_REQUIRE(((uintptr_t)out | (uintptr_t)c) % 4 == 0, "mcr_linear_planes_dot: out and c must be 4-byte aligned");
    const Planes X{(_Float16*)Xh, (_Float16*)Xl, ldx};                  // (read only)
    const WPlanes W{(const _Float16*)Wh, (const _Float16*)Wl, ldw, wscale_inv};
    launch_linear3p_dot((hipStream_t)stream, X, W, {bias, gelu ? ACT_GELU : ACT_NONE}, M, K, v, c, gelu2 ? ACT_GELU : ACT_NONE, out, n_planes);
    MCR_LAUNCH_CHECK("mcr_linear_planes_dot");
    return 0;
}

}  // extern "C"
