// SconeVis.forward / PCTransformer.forward / SconeOcc.forward composed from the gfx950 building blocks
// (nn_kernels.hip, knn.hip) behind single C-ABI entry points (include/macarons_hip.h).
//
// Reference (file:line, upstream tree):
//   macarons/networks/Attention.py:98-128   Embedding.forward      (linear-GELU-linear, optional cloud max, concat x)
//   macarons/networks/Attention.py:278-300  Encoder.forward        (pre-LN MHSA + residual, pre-LN FF + residual)
//   macarons/networks/SconeVis.py:121-162   SconeVis.forward
//   macarons/networks/SconeOcc.py:104-130   PCTransformer.forward
//   macarons/networks/SconeOcc.py:250-347   SconeOcc.forward
// Only the reference's default architecture hyper-parameters are implemented on the HIP path (every call site
// uses them); the Python host classes refuse other configurations loudly.
// The weight tables the entries read and the arena their workspaces are carved from are described once, in net_layout.h; each
// entry's scratch is a struct with one carve function below, which its *_workspace_bytes measures.
#include "nn_kernels.h"
#include "net_layout.h"
#include <cstdlib>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace mcr {

// 1: local_pct.hip exact-fp32 MFMA; 5: local_pct5.hip split-precision bf16 hi/mid/lo (6 MFMAs per product, whole fp32
// range); 6 (default): local_pct6.hip two-term fp16 split (3 MFMAs per product); 7 (OPT-IN, per call only -- never a process
// default): local_pct7.hip, ONE fp16 plane per matrix operand (1 MFMA per product), BASELINE.json config 3's 16-bit matrix
// path with its own stated tolerance (tests/test_variant7_gpu.py).  Each has its own blob format.
#ifdef MCR_DEV_LOCAL_PCT8      // dev builds only (tools/build_variant.py with tools/experiments/local_pct8.hip): the shelved register-resident kernel as variant 8
void launch_local_pct8(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob);
#define MCR_VARIANT8_OK(v) ((v) == 8)
#else
#define MCR_VARIANT8_OK(v) false
#endif
// The numerics variant is a property of a CALL, not of the process: every network entry point opens a VariantScope, which fixes the
// variant of that call on the calling thread -- the one-shot value mcr_call_variant(v) left for it (the per-call argument of the ABI:
// "the next network entry point on this thread runs on v"), else the process default (mcr_set_local_pct_variant / env
// MCR_LOCAL_PCT_VARIANT).  Two host threads, or two models on different variants, cannot see each other's choice, and a failed
// call cannot leave a flipped switch behind (round 4 flipped a process-global around the range-guard fallback).
static int g_default_variant = []() {                   // env MCR_LOCAL_PCT_VARIANT picks the start-up value (testing: whole suites on a variant)
    const char* e = getenv("MCR_LOCAL_PCT_VARIANT");
    const int v = e ? atoi(e) : 6;
    return (v == 1 || v == 5 || v == 6) ? v : 6;
}();
static thread_local int t_next_variant = 0;             // one-shot: consumed by the next VariantScope of this thread
static thread_local int t_variant = 0;                  // the variant of the entry point running on this thread
static thread_local int t_scope_depth = 0;              // (an entry point may call another: the outermost scope decides)
struct VariantScope {
    VariantScope() {
        if (t_scope_depth++ == 0) {
            t_variant = t_next_variant ? t_next_variant : g_default_variant;
            t_next_variant = 0;
        }
    }
    ~VariantScope() {
        if (--t_scope_depth == 0) t_variant = 0;
    }
};
#define g_local_pct_variant (t_variant ? t_variant : g_default_variant)
// Variant 7 shares variant 6's routes (operands as fp16 planes in HBM, the same range guard); what differs is how many planes a
// product multiplies: matrix_planes() = 1 on variant 7 (the high planes alone; low planes are neither written nor read where
// the single-plane kernels exist: the local transformers and the SconeOcc head), 2 on variant 6.
static inline bool fp16_planes_variant() { return g_local_pct_variant == 6 || g_local_pct_variant == 7; }
static inline int matrix_planes() { return g_local_pct_variant == 7 ? 1 : 2; }
// rows-per-sequence argument of launch_linear for the encoders of the 2048-token networks (SconeVis, SconeOcc's global
// transformer): on the split-precision variants (5, 6) their GEMMs take the split-precision kernel for EVERY launch size (negative
// argument = "choose on the layer's shape"; its column-tile width follows the launch, which does not change a single bit) -- one
// sequence costs the same as on the fp32 kernels, 8 or 30 sequences in one launch (scene batch, the neighbour cameras of a MACARONS
// decision) run 1.3x faster, and a sequence's result still does not depend on how many share the launch.  Variant 1 = exact fp32
// everywhere.  The wide layers behind the encoders (SconeVis fc1 / fc2, the global transformer's lin0) take the same route.
static inline int64_t seq_route(int64_t L) { return g_local_pct_variant >= 5 ? -L : L; }

// long-sequence attention: P V on fp16 hi/lo pairs (nn_kernels.hip: PVH) on the fp16-split variants, fp32 MFMA on the others
static inline bool attn_pv_half() { return fp16_planes_variant(); }

// Encoder GEMMs of the long-sequence networks on fp16 hi/lo PLANES (variants 6 and 7, sequences of >= 512 tokens; shorter ones take the
// bf16 x 6 kernels as on variant 5): the GEMM inputs are split once where they are produced -- LayerNorm writes planes, the FF's
// first GEMM writes planes, the attention output is split in one pass -- and every operand reaches LDS by DMA (linear3p.hip): no
// split and no staging registers inside the GEMMs, three MFMAs per product instead of six.  Chosen on the sequence length alone, so a
// cloud's result does not depend on how many clouds share the launch.  Needs |activation| < 65504 like the rest of variant 6: the
// occupancy / harmonics that come out non-finite otherwise are what the range guards look at.  The layers either side of the encoders
// (the embeddings' second layer, the final LayerNorm and the fc / lin0 layers behind it) are on the same path under the same condition.
static inline bool enc_planes(int L, int E) { return fp16_planes_variant() && L >= 512 && E % 32 == 0; }

// The weight planes of one layer: the host-built ones (`given`, scale 1 / given_inv; one split per parameter version instead of per call)
// when the table has them, else planes split here into `scratch` with the fixed 2^8 scale (|w| < 255).  Np, Kp (optional): the layer
// zero-padded to [2][Np][Kp]; its padded bias then goes behind the planes and replaces *bias_p -- on entry the host-built one.
static WPlanes weight_planes(hipStream_t s, const void* given, float given_inv, const LinW& lin, int64_t ldw, int N, int K, void* scratch,
                             int Np = 0, int Kp = 0, const float** bias_p = nullptr) {
    const bool pad = Np > 0;
    if (!pad) { Np = N; Kp = K; }
    if (!given) {
        if (pad) {
            float* bp = reinterpret_cast<float*>(scratch) + (size_t)Np * Kp;               // behind the [2][Np][Kp] halves
            launch_pad_weights(s, lin.w, ldw, lin.b, scratch, bp, N, K, Np, Kp);
            *bias_p = bp;
        } else
            launch_split_weights(s, lin.w, ldw, scratch, N, K);
        given = scratch;
        given_inv = WSPLIT_INV;
    }
    const _Float16* h = (const _Float16*)given;
    return {h, h + (size_t)Np * Kp, Kp, given_inv};
}

// The planes live in the encoder's own scratch (planes_over: an fp32 row = two fp16 rows): h <- planes of LayerNorm(x) / of the planes
// attention's output, ff <- planes of the FF's hidden layer; the weights' planes (split per call unless the host built them) go to
// whichever of ff / qkv is idle.  L >= 512 makes every region large enough for them.
static void run_encoder_planes(hipStream_t s, const EncW& w, float* x, float* h, float* qkv, float* ff, int64_t S, int L, int E, int H,
                               const int* lens) {
    const int64_t T = S * L;
    const int dqk = E / 4, W3 = 2 * dqk + E;
    const bool attn_planes = attention_planes_applicable(H, dqk, E, W3);
    // 1 on variant 7 (with head dims the planes attention covers: the default architectures): the LayerNorms' low plane is neither written nor read
    const int np = attn_planes ? matrix_planes() : 2;
    const Planes hP = planes_over(h, T, E), nP = hP.keep(np);                                // nP: what the LayerNorms write
    const Planes fP = planes_over(ff, T, 2 * E);
    const size_t ff_floats = (size_t)T * 2 * E;                                              // (ff is free during the attention: key-split scratch)
    launch_layernorm_planes(s, {x, E}, w.n1g, w.n1b, nP, T, E);                              // Attention.py:287
    const WPlanes Wq = weight_planes(s, w.p_qkv, WSPLIT_INV, w.qkv, E, W3, E, ff);
    Planes aP = planes_over(qkv, T, E);                                                      // the attention's result
    if (attn_planes) {
        // q | k | v leave the projection as planes [2][T][W3] over qkv (:186-188); the attention stages K / V tiles by DMA (:191-198) and
        // writes its result as planes over h (the LayerNorm's, consumed by then).  One block per (query tile, head, sequence) whatever S is
        // (a cloud's result must not depend on how many clouds share the launch): a batch of clouds saves the combine pass and the fp32
        // parts of the key-split form (0.23 ms of a MACARONS decision); one cloud alone pays 13 us per attention for it (41 instead of
        // 23 + 5 us, hidden beside the local transformers in an NBV step).
        const Planes qP = planes_over(qkv, T, W3);
        launch_linear3p(s, nP, Wq, {w.qkv.b, ACT_NONE}, qP, T, W3, E, np);
        aP = hP;
        launch_attention_planes(s, qP, {h, E}, aP, S, L, H, dqk, E, lens, {ff, ff_floats, /*mode=*/0}, np);
    } else {
        launch_linear3p(s, nP, Wq, {w.qkv.b, ACT_NONE}, {qkv, W3}, T, W3, E, np);            // :186-188
        // attention: fp32 parts in h / ff (key-split scratch); its combine pass writes the result straight as planes into qkv (free by then)
        if (!launch_attention(s, {qkv, W3}, {h, E}, S, L, H, dqk, E, lens, {ff, ff_floats, 1}, attn_pv_half(), aP))   // :191-198
            launch_split_to_planes(s, {h, E}, aP, T, E);
    }
    const WPlanes Wo = weight_planes(s, w.p_out, WSPLIT_INV, w.out, E, E, E, ff);
    launch_linear3p(s, aP, Wo, {w.out.b, ACT_NONE, {x, E}}, {x, E}, T, E, E, np);            // :201-202 + residual :290
    launch_layernorm_planes(s, {x, E}, w.n2g, w.n2b, nP, T, E);                              // :293
    const WPlanes W1 = weight_planes(s, w.p_ff1, WSPLIT_INV, w.ff1, E, 2 * E, E, qkv);
    launch_linear3p(s, nP, W1, {w.ff1.b, ACT_GELU}, fP, T, 2 * E, E, np);                    // :232 (planes out)
    const WPlanes W2 = weight_planes(s, w.p_ff2, WSPLIT_INV, w.ff2, 2 * E, E, 2 * E, qkv);
    launch_linear3p(s, fP, W2, {w.ff2.b, ACT_NONE, {x, E}}, {x, E}, T, E, 2 * E, np);        // :235 + residual :298
}

// x <- Encoder(x)  in place.  x [T, E]; scratch h [T, E], qkv [T, 2*dqk + E], ff [T, 2E]
static void run_encoder(hipStream_t s, const EncW& w, float* x, float* h, float* qkv, float* ff, int64_t S, int L, int E,
                        int H, const int* lens = nullptr) {
    const int64_t T = S * L;
    const int dqk = E / 4, W3 = 2 * dqk + E;
    if (enc_planes(L, E)) {
        run_encoder_planes(s, w, x, h, qkv, ff, S, L, E, H, lens);
        return;
    }
    const int64_t route = seq_route(L);      // every GEMM of the networks routes (fp32 vs split precision) on the rows of ONE sequence, not on T: see launch_linear
    const size_t ff_floats = (size_t)T * 2 * E;
    launch_layernorm(s, x, E, w.n1g, w.n1b, h, E, T, E);                                                   // Attention.py:287
    launch_linear(s, {h, E}, {w.qkv.w, E}, {w.qkv.b, ACT_NONE}, {qkv, W3}, T, W3, E, route);               // :186-188
    launch_attention(s, {qkv, W3}, {h, E}, S, L, H, dqk, E, lens, {ff, ff_floats, 1}, attn_pv_half());     // :191-198 (ff is free here: key-split scratch)
    launch_linear(s, {h, E}, {w.out.w, E}, {w.out.b, ACT_NONE, {x, E}}, {x, E}, T, E, E, route);           // :201-202 + residual :290
    launch_layernorm(s, x, E, w.n2g, w.n2b, h, E, T, E);                                                   // :293
    launch_linear(s, {h, E}, {w.ff1.w, E}, {w.ff1.b, ACT_GELU}, {ff, 2 * E}, T, 2 * E, E, route);          // :232
    launch_linear(s, {ff, 2 * E}, {w.ff2.w, 2 * E}, {w.ff2.b, ACT_NONE, {x, E}}, {x, E}, T, E, 2 * E, route);   // :235 + residual :298
}

// ---- PCTransformer (SconeOcc.py:45-130): S sequences of L points (pts_dim 3), E = 128, 2 encoders, 4 heads ----
constexpr int PCT_E = 128, PCT_INNER = 125;
// The scratch of a stack of encoders of width E over T tokens (PCTransformer: E = 128; SconeVis: E = 256): the residual stream x and
// the encoder's h [T, E], qkv [T, 2*dqk + E] (dqk = E / 4), ff [T, 2E]
struct EncScratch { float *x, *h, *qkv, *ff; };
static EncScratch carve_enc(Arena& a, int64_t T, int E) {
    EncScratch w;
    w.x = a.f(T * E);
    w.h = a.f(T * E);
    w.qkv = a.f(T * (E + E / 2));
    w.ff = a.f(T * 2 * E);
    return w;
}
// feat[s*ld_feat + 0 : feature_dim] ; feature_dim = 2 * half (max || avg)
// lens (optional, device int per sequence): sequence s consists of its first lens[s] rows (zero-padded batch of clouds of
// different sizes): attention keys and the pooling stop there
static void run_pct(hipStream_t s, const PctW& w, const float* pc, float* feat, int64_t ld_feat, int64_t S, int L, int half,
                    const EncScratch& ws, const int* lens = nullptr) {
    const int64_t T = S * L;
    float *x = ws.x, *h = ws.h, *qkv = ws.qkv, *ff = ws.ff;
    const bool planes = enc_planes(L, PCT_E) && half % 4 == 0;
    const int np = matrix_planes();                       // 1 on variant 7: the GEMMs below multiply the high planes alone
    const Planes hP = planes_over(h, T, PCT_E);
    // Embedding (Attention.py:98-128): linear1 3->125, GELU, linear2 125->125, concat raw input -> 128
    if (planes) {
        // the 125-wide inner layer padded with exact zeros to the planes GEMM's K = 128: linear1 writes planes, linear2 multiplies them
        // (output columns 125..127 = 0 + 0, then overwritten by the raw input)
        launch_linear_smallk_planes(s, {pc, 3}, w.l1.w, w.l1.b, ACT_GELU, hP, T, PCT_INNER, 3, PCT_E);
        const float* b2 = w.b_l2p;
        const WPlanes W2 = weight_planes(s, w.p_l2, WSPLIT_INV, w.l2, PCT_INNER, PCT_INNER, PCT_INNER, ff, PCT_E, PCT_E, &b2);
        launch_linear3p(s, hP, W2, {b2, ACT_NONE}, {x, PCT_E}, T, PCT_E, PCT_E, np);
    } else {
        launch_linear(s, {pc, 3}, {w.l1.w, 3}, {w.l1.b, ACT_GELU}, {h, PCT_INNER}, T, PCT_INNER, 3, L);
        launch_linear(s, {h, PCT_INNER}, {w.l2.w, PCT_INNER}, {w.l2.b, ACT_NONE}, {x, PCT_E}, T, PCT_INNER, PCT_INNER, L);
    }
    launch_copy2d(s, pc, 3, x + PCT_INNER, PCT_E, T, 3);
    for (int e = 0; e < 2; ++e) run_encoder(s, w.enc[e], x, h, qkv, ff, S, L, PCT_E, 4, lens);
    if (planes) {                                                                            // SconeOcc.py:119-122 on planes
        launch_layernorm_planes(s, {x, PCT_E}, w.ng, w.nb, hP.keep(np), T, PCT_E);
        const WPlanes W0 = weight_planes(s, w.p_lin0, WSPLIT_INV, w.lin0, PCT_E, half, PCT_E, qkv);
        launch_linear3p(s, hP, W0, {w.lin0.b, ACT_NONE}, {ff, half}, T, half, PCT_E, np);
    } else {
        launch_layernorm(s, x, PCT_E, w.ng, w.nb, h, PCT_E, T, PCT_E);                      // SconeOcc.py:119
        launch_linear(s, {h, PCT_E}, {w.lin0.w, PCT_E}, {w.lin0.b, ACT_NONE}, {ff, half}, T, half, PCT_E, seq_route(L));   // :122
    }
    launch_pool_max_avg(s, ff, half, feat, ld_feat, S, L, half, lens);                       // :124-126
}

// *flag |= 1 if any of x[0..n) is inf / NaN (the flag is the caller's: cleared by the caller, OR'ed here)
__global__ void nonfinite_flag_kernel(const float* __restrict__ x, long long n, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        bad |= !(fabsf(x[i]) <= 3.4028234663852886e38f);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
static void launch_nonfinite_flag(hipStream_t s, const float* x, int64_t n, int* flag) {
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 1024)), dim3(256), 0, s, x, (long long)n, flag);
}

// ---- SconeOcc head on fp16 hi/lo planes end to end (variant 6; linear3p.hip): every activation is split once where it is produced
// (local_pct6's pooled features, the GEMM epilogues), every operand reaches LDS by DMA.  Scratch (the caller's regions, same
// bytes as the fp32 layout): featP = planes [2][T][1344] fp16, h1P = [2][T][512] fp16 (first used as [2][T][256] for the
// x-embedding), h2 = fp32 [T][256] (first half first used for xe1's fp32 output, second half for its planes).
struct HeadScratch { _Float16* featP; _Float16* h1P; float* h2; void* wplanes; };
// weight planes of head layer `which` (0 xe2, 1 xe3, 2 lin1's columns 512..1855, 3 lin2: the order of the host's pre-split planes)
static WPlanes head_weight_planes(hipStream_t s, int which, const LinW& lin, int64_t ldw, int N, int K, const void* const* head_planes,
                                  const float* head_inv_scales, void* wplanes) {
    const bool pre = head_planes && head_planes[which] && head_inv_scales[which] > 0.f;
    return weight_planes(s, pre ? head_planes[which] : nullptr, pre ? head_inv_scales[which] : 0.f, lin, ldw, N, K, wplanes);
}
// the part of the planes head that needs nothing but the queries: x embedding 3 -> 128 -> 256 -> 512 (GELU each, SconeOcc.py:35-42)
// into columns 768.. of the feature planes, the view harmonics into columns 1280..
static void run_x_embedding_planes(hipStream_t s, const float* x, const float* view_harmonics, int64_t T, const LinW& xe1, const LinW& xe2,
                                   const LinW& xe3, const void* const* head_planes, const float* head_inv_scales, const HeadScratch& w) {
    const Planes fP = planes_over(w.featP, T, 1344), hP = planes_over(w.h1P, T, 256);
    const Planes x1 = planes_over(w.h2 + T * 128, T, 128);
    const int np = matrix_planes();                      // 1 on variant 7: the low planes below are neither written (GEMM epilogues) nor read
    launch_linear_smallk_planes(s, {x, 3}, xe1.w, xe1.b, ACT_GELU, x1, T, 128, 3, /*Np=*/0);   // (planes directly: no fp32 rows, no split pass)
    const WPlanes W2 = head_weight_planes(s, 0, xe2, 128, 256, 128, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, x1, W2, {xe2.b, ACT_GELU}, hP, T, 256, 128, np);
    const WPlanes W3 = head_weight_planes(s, 1, xe3, 256, 512, 256, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, hP, W3, {xe3.b, ACT_GELU}, fP.cols(768), T, 512, 256, np);
    if (view_harmonics) launch_split_to_planes(s, {view_harmonics, 64}, fP.cols(1280).keep(np), T, 64);   // (NULL: the caller splits them later)
}

// x_done: the x-embedding part has been queued elsewhere (the side stream: the join covers it)
template <class Join>
static void run_head_planes(hipStream_t s, const float* x, const float* view_harmonics, int64_t T, const LinW& xe1, const LinW& xe2,
                            const LinW& xe3, const LinW& lin1, const LinW& lin2, const LinW& lin3, const float* gbias,
                            int64_t rows_per_group, const int* row_group, const void* const* head_planes, const float* head_inv_scales,
                            const HeadScratch& w, float* out, Join join, bool x_done = false) {
    const Planes fP = planes_over(w.featP, T, 1344), hP = planes_over(w.h1P, T, 512);
    const int np = matrix_planes();
    if (!x_done) run_x_embedding_planes(s, x, view_harmonics, T, xe1, xe2, xe3, head_planes, head_inv_scales, w);
    join();                                               // the global feature (side stream) is needed from here on
    // head MLP 1856 -> 512 -> 256 -> 1, GELU after every layer incl. the last (SconeOcc.py:334-345); the global 512 columns are gbias
    const WPlanes W1 = head_weight_planes(s, 2, {lin1.w + 512, lin1.b}, 1856, 512, 1344, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, fP, W1, {lin1.b, ACT_GELU, {}, {gbias, rows_per_group, row_group}}, hP, T, 512, 1344, np);
    const WPlanes W2 = head_weight_planes(s, 3, lin2, 512, 256, 512, head_planes, head_inv_scales, w.wplanes);
    // 512 -> 256 (GELU) -> 1 (GELU) in one launch: the block owns all 256 features of its rows and dots them with linear3.weight
    launch_linear3p_dot(s, hP, W2, {lin2.b, ACT_GELU}, T, 512, lin3.w, lin3.b, ACT_GELU, out, np);
}

}  // namespace mcr

using namespace mcr;

extern "C" {

// ---- individual blocks (used by the host mirrors of Attention.py's modules and by the block-level tests) ----
int mcr_linear(const float* X, int64_t ldx, const float* W, const float* bias, const float* residual, int64_t ldr, float* Y,
               int64_t ldy, int64_t M, int N, int K, int gelu, void* stream) {
    VariantScope variant_scope_;
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
    MCR_REQUIRE(qkv && out, "mcr_attention: null pointer");
    MCR_REQUIRE(S > 0 && L > 0, "mcr_attention: empty problem");
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "mcr_attention: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)",
                n_heads, qk_dim, v_dim);
    MCR_REQUIRE(L == 16 || S <= 65535, "mcr_attention: too many long sequences");
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "mcr_attention: leading dimension too small");
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, nullptr, AttnSplit{}, attn_pv_half());
    MCR_LAUNCH_CHECK("mcr_attention");
    return 0;
}

int mcr_attention_masked(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                         const unsigned char* mask, int64_t mask_seq_stride, int64_t mask_head_stride, int64_t mask_query_stride,
                         void* workspace, size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(qkv && out && mask, "mcr_attention_masked: null pointer");
    MCR_REQUIRE(S > 0 && L > 0, "mcr_attention_masked: empty problem");
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "mcr_attention_masked: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)",
                n_heads, qk_dim, v_dim);
    MCR_REQUIRE(mask_seq_stride >= 0 && mask_head_stride >= 0 && mask_query_stride >= 0, "mcr_attention_masked: negative mask stride");
    MCR_REQUIRE(L == 16 || S <= 32767, "mcr_attention_masked: too many long sequences");
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "mcr_attention_masked: leading dimension too small");
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
    MCR_REQUIRE(qkv && out, "mcr_attention_ws: null pointer");
    MCR_REQUIRE(S > 0 && L > 0, "mcr_attention_ws: empty problem");
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "mcr_attention_ws: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)",
                n_heads, qk_dim, v_dim);
    MCR_REQUIRE(L == 16 || S <= 32767, "mcr_attention_ws: too many long sequences");
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "mcr_attention_ws: leading dimension too small");
    const AttnSplit split{(float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, /*mode=*/-1};
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, nullptr, split, attn_pv_half());
    MCR_LAUNCH_CHECK("mcr_attention_ws");
    return 0;
}

// TEST entry: launch_attention as the encoders call it (networks.hip: run_encoder*, pct_bwd.hip) -- per-sequence lengths and an explicit
// split mode.  Adds no kernel.
int mcr_attention_lens(const float* qkv, int64_t ldq, float* out, int64_t ldo, int64_t S, int64_t L, int n_heads, int qk_dim, int v_dim,
                       const int* lens, int split_mode, void* workspace, size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(qkv && out, "mcr_attention_lens: null pointer");
    MCR_REQUIRE(S > 0 && L > 0, "mcr_attention_lens: empty problem");
    MCR_REQUIRE(n_heads == 4 && ((qk_dim == 32 && v_dim == 128) || (qk_dim == 64 && v_dim == 256)),
                "mcr_attention_lens: supported head layouts are 4 heads with (qk,v) = (32,128) or (64,256); got %d heads (%d,%d)",
                n_heads, qk_dim, v_dim);
    MCR_REQUIRE(split_mode >= -1 && split_mode <= 1, "mcr_attention_lens: split_mode must be 1, 0 or -1 (got %d)", split_mode);
    // (with lens a 16-token sequence runs the matrix-pipe kernel too: one grid.z slot per sequence)
    MCR_REQUIRE((L == 16 && !lens) || S <= 32767, "mcr_attention_lens: too many long sequences");
    MCR_REQUIRE(ldq >= 2 * qk_dim + v_dim && ldo >= v_dim, "mcr_attention_lens: leading dimension too small");
    // the launcher drops to the unsplit form when the scratch is short; here a split that was asked for must be possible
    if (split_mode != 0 && L >= 512 && (workspace || split_mode == 1)) {
        MCR_REQUIRE(workspace && workspace_bytes >= mcr_attention_workspace_bytes(S, L, n_heads, v_dim),
                    "mcr_attention_lens: workspace too small for the key split (%zu bytes, %zu needed)", workspace ? workspace_bytes : (size_t)0,
                    mcr_attention_workspace_bytes(S, L, n_heads, v_dim));
        MCR_REQUIRE((uintptr_t)workspace % 16 == 0, "mcr_attention_lens: the workspace must be 16-byte aligned");
    }
    const AttnSplit split{(float*)workspace, workspace ? workspace_bytes / sizeof(float) : 0, split_mode};
    launch_attention((hipStream_t)stream, {qkv, ldq}, {out, ldo}, S, (int)L, n_heads, qk_dim, v_dim, lens, split, attn_pv_half());
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

// TEST entries: the padded-sequence forms of the two launchers above, as run_pc_transformer and the SconeVis embedding call them
// (lens: device int [S], may be NULL).  They add no kernel.
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

// ---- the planes GEMMs of variants 6 / 7 (linear3p.hip) as blocks of their own: bring-up / test entries.  The networks call the
// launchers directly; these forward to the same launchers after checking on the host what the kernels assume.
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

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
    // the operand planes are the sources of 16-byte DMA; bias rows are read by 16-byte loads at columns that are multiples of 4
    MCR_REQUIRE(al16(Xh) && al16(Wh) && (n_planes == 1 || (al16(Xl) && al16(Wl))), "mcr_linear_planes: operand planes must be 16-byte aligned");
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
    MCR_REQUIRE(al16(Xh) && al16(Wh) && (n_planes == 1 || (al16(Xl) && al16(Wl))), "mcr_linear_planes_dot: operand planes must be 16-byte aligned");
    MCR_REQUIRE(al16(bias) && al16(v), "mcr_linear_planes_dot: bias and v must be 16-byte aligned");
    MCR_REQUIRE(((uintptr_t)out | (uintptr_t)c) % 4 == 0, "mcr_linear_planes_dot: out and c must be 4-byte aligned");
    const Planes X{(_Float16*)Xh, (_Float16*)Xl, ldx};                  // (read only)
    const WPlanes W{(const _Float16*)Wh, (const _Float16*)Wl, ldw, wscale_inv};
    launch_linear3p_dot((hipStream_t)stream, X, W, {bias, gelu ? ACT_GELU : ACT_NONE}, M, K, v, c, gelu2 ? ACT_GELU : ACT_NONE, out, n_planes);
    MCR_LAUNCH_CHECK("mcr_linear_planes_dot");
    return 0;
}

int mcr_get_local_pct_variant(void);
int mcr_local_pct_blob_floats(void) { return local_pct_blob_floats(); }
int mcr_local_pct3_blob_floats(void) { return local_pct5_blob_floats(); }
int mcr_local_pct6_blob_floats(void) { return local_pct6_blob_floats(); }
int mcr_local_pct7_blob_floats(void) { return local_pct7_blob_floats(); }

int mcr_set_local_pct_variant(int v) {
    MCR_REQUIRE(v == 1 || v == 5 || v == 6 || MCR_VARIANT8_OK(v), "mcr_set_local_pct_variant: the process default must be 1, 5 or 6 (got %d; 7, the opt-in 16-bit matrix path, is per call only: mcr_call_variant)", v);
    g_default_variant = v;
    return 0;
}
int mcr_get_local_pct_variant(void) { return g_default_variant; }
int mcr_call_variant(int v) {
    MCR_REQUIRE(v == 0 || v == 1 || v == 5 || v == 6 || v == 7 || MCR_VARIANT8_OK(v),
                "mcr_call_variant: variant must be 0 (default), 1, 5, 6 or 7 (the opt-in 16-bit matrix path) (got %d)", v);
    t_next_variant = v;
    return 0;
}
// P (optional): the features as fp16 planes (row stride ld halves) instead of fp32 rows of feat
static void run_local_pct(hipStream_t s, const float* offs, float* feat, int64_t ld, int64_t S, const float* blob, Planes P = Planes{}) {
    if (g_local_pct_variant == 1) launch_local_pct(s, offs, feat, ld, S, blob);
    else if (g_local_pct_variant == 5) launch_local_pct5(s, offs, feat, ld, S, blob);
#ifdef MCR_DEV_LOCAL_PCT8
    else if (g_local_pct_variant == 8) launch_local_pct8(s, offs, feat, ld, S, blob);
#endif
    else if (g_local_pct_variant == 7) launch_local_pct7(s, offs, feat, ld, S, blob, P.h);   // ONE plane out when P.h is set
    else launch_local_pct6(s, offs, feat, ld, S, blob, P.h, P.l);       // planes out (variant 6 only) when P.h is set
}

int mcr_local_pct_forward(const float* offsets, float* features, int64_t ld_features, int64_t S, const float* blob,
                          void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(offsets && features && blob, "mcr_local_pct_forward: null pointer");
    MCR_REQUIRE(S > 0 && ld_features >= 256, "mcr_local_pct_forward: bad sizes");
    MCR_REQUIRE((reinterpret_cast<uintptr_t>(blob) & 15) == 0, "mcr_local_pct_forward: blob must be 16-byte aligned");
    run_local_pct((hipStream_t)stream, offsets, features, ld_features, S, blob);
    MCR_LAUNCH_CHECK("mcr_local_pct_forward");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
constexpr size_t PCT_WS_SLACK = 4096;
size_t mcr_pc_transformer_workspace_bytes(int64_t S, int64_t L) { return measure(carve_enc, S * L, PCT_E) + PCT_WS_SLACK; }

int mcr_pc_transformer_forward(const float* pc, float* features, int64_t S, int64_t L, int feature_dim,
                               const float* const* weights, int n_weights, void* workspace, size_t workspace_bytes,
                               void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(pc && features && weights, "mcr_pc_transformer_forward: null pointer");
    if (check_table("mcr_pc_transformer_forward", PCT_TABLE, weights, n_weights, n_weights)) return 1;
    MCR_REQUIRE(S > 0 && L > 0, "mcr_pc_transformer_forward: empty problem");
    MCR_REQUIRE(feature_dim == 256 || feature_dim == 512, "mcr_pc_transformer_forward: feature_dim must be 256 or 512");
    MCR_REQUIRE(L == 16 || S <= 65535, "mcr_pc_transformer_forward: too many long sequences");
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_pc_transformer_workspace_bytes(S, L),
                "mcr_pc_transformer_forward: workspace too small");
    PctW w = read_pct(weights);
    read_pct_tails(w, PCT_TABLE, weights, n_weights);
    Arena a{(char*)workspace, workspace_bytes};
    const EncScratch ws = carve_enc(a, S * L, PCT_E);
    MCR_REQUIRE(a.ok(), "mcr_pc_transformer_forward: workspace too small");
    run_pct((hipStream_t)stream, w, pc, features, feature_dim, S, (int)L, feature_dim / 2, ws);
    MCR_LAUNCH_CHECK("mcr_pc_transformer_forward");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// SconeVis.forward (SconeVis.py:121-162): E = 256, 3 encoders, 4 heads, view_state_mode "end".
constexpr int VIS_E = 256, VIS_F = 126;
constexpr size_t VIS_WS_SLACK = 4096;

size_t mcr_scone_vis_workspace_bytes(int64_t B, int64_t N) { return measure(carve_enc, B * N, VIS_E) + VIS_WS_SLACK; }

int mcr_scone_vis_forward(const float* pts, const float* view_harmonics, float* out, int64_t B, int64_t N,
                          const float* const* weights, int n_weights, const int* lengths, void* workspace,
                          size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(pts && view_harmonics && out && weights, "mcr_scone_vis_forward: null pointer");
    if (check_table("mcr_scone_vis_forward", VIS_TABLE, weights, n_weights, n_weights)) return 1;
    MCR_REQUIRE(B > 0 && N > 0 && B <= 65535, "mcr_scone_vis_forward: bad problem size B=%ld N=%ld", (long)B, (long)N);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_vis_workspace_bytes(B, N), "mcr_scone_vis_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const VisW w = read_vis_table(weights, n_weights);
    const LinW &l1 = w.l1, &l2 = w.l2, &fc1 = w.fc1, &fc2 = w.fc2, &fc3 = w.fc3;

    const int64_t T = B * N;
    Arena a{(char*)workspace, workspace_bytes};
    const EncScratch ws = carve_enc(a, T, VIS_E);
    MCR_REQUIRE(a.ok(), "mcr_scone_vis_forward: workspace too small");
    float *x = ws.x, *h = ws.h, *qkv = ws.qkv, *ff = ws.ff;
    const bool planes = enc_planes((int)N, VIS_E);
    const int np = matrix_planes();                       // 1 on variant 7: the GEMMs below multiply the high planes alone
    const Planes hP = planes_over(h, T, VIS_E), h128 = planes_over(h, T, 128);                  // planes [2][T][256] / [2][T][128] over h
    // Embedding: 4 -> 126 GELU -> 126, || cloud-wide max (126) || raw input (4)  = 256   (Attention.py:98-128)
    if (planes) {
        // the 126-wide inner layer padded with exact zeros to K = 128: linear1 writes planes, linear2 multiplies them (its output
        // columns 126, 127 = 0 + 0 are overwritten by the cloud-wide max below)
        launch_linear_smallk_planes(s, {pts, 4}, l1.w, l1.b, ACT_GELU, h128, T, VIS_F, 4, 128);
        const float* b2 = w.b_l2p;
        const WPlanes W2 = weight_planes(s, w.p_l2, WSPLIT_INV, l2, VIS_F, VIS_F, VIS_F, ff, 128, 128, &b2);
        launch_linear3p(s, h128, W2, {b2, ACT_NONE}, {x, VIS_E}, T, 128, 128, np);
    } else {
        launch_linear(s, {pts, 4}, {l1.w, 4}, {l1.b, ACT_GELU}, {h, VIS_F}, T, VIS_F, 4, N);
        launch_linear(s, {h, VIS_F}, {l2.w, VIS_F}, {l2.b, ACT_NONE}, {x, VIS_E}, T, VIS_F, VIS_F, N);
    }
    launch_colmax_broadcast(s, x, VIS_E, x + VIS_F, VIS_E, B, (int)N, VIS_F, lengths, pts, 4, 4, x + 2 * VIS_F);   // (+ the raw input columns)
    for (int e = 0; e < 3; ++e) run_encoder(s, w.enc[e], x, h, qkv, ff, B, (int)N, VIS_E, 4, lengths);   // SconeVis.py:139-140
    if (planes) {
        // :143-152 on planes: LayerNorm -> planes; fc1 (GELU) writes columns 0..191 of the next operand's planes, the view harmonics are
        // split into columns 192..255; fc2 (GELU) writes planes over h (the LayerNorm's are consumed); fc3 leaves fp32.  Weight planes:
        // split per call into the idle qkv region, one behind the other
        launch_layernorm_planes(s, {x, VIS_E}, w.ng, w.nb, hP.keep(np), T, VIS_E);
        _Float16* q = reinterpret_cast<_Float16*>(qkv);
        const WPlanes W1 = weight_planes(s, w.p_fc1, WSPLIT_INV, fc1, VIS_E, 192, VIS_E, q);
        const WPlanes W2 = weight_planes(s, w.p_fc2, WSPLIT_INV, fc2, VIS_E, 128, VIS_E, q + 2 * 192 * VIS_E);
        const WPlanes W3 = weight_planes(s, w.p_fc3, WSPLIT_INV, fc3, 128, 64, 128, q + 2 * (192 + 128) * VIS_E);
        const Planes fP = planes_over(ff, T, VIS_E);
        launch_linear3p(s, hP, W1, {fc1.b, ACT_GELU}, fP, T, 192, VIS_E, np);
        launch_split_to_planes(s, {view_harmonics, 64}, fP.cols(192).keep(np), T, 64);
        launch_linear3p(s, fP, W2, {fc2.b, ACT_GELU}, h128, T, 128, VIS_E, np);
        launch_linear3p(s, h128, W3, {fc3.b, ACT_NONE}, {out, 64}, T, 64, 128, np);
    } else {
        launch_layernorm(s, x, VIS_E, w.ng, w.nb, h, VIS_E, T, VIS_E);                                   // :143
        // fc1 256->192 GELU, || view_harmonics (64), fc2 256->128 GELU, fc3 128->64                  (:146-152)
        launch_linear(s, {h, VIS_E}, {fc1.w, VIS_E}, {fc1.b, ACT_GELU}, {ff, VIS_E}, T, 192, VIS_E, seq_route(N));
        launch_copy2d(s, view_harmonics, 64, ff + 192, VIS_E, T, 64);
        launch_linear(s, {ff, VIS_E}, {fc2.w, VIS_E}, {fc2.b, ACT_GELU}, {h, 128}, T, 128, VIS_E, seq_route(N));
        launch_linear(s, {h, 128}, {fc3.w, 128}, {fc3.b, ACT_NONE}, {out, 64}, T, 64, 128, N);
    }
    MCR_LAUNCH_CHECK("mcr_scone_vis_forward");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// SconeOcc.forward (SconeOcc.py:250-347).  The host supplies the already down-sampled clouds (it consumes
// torch's CPU generator exactly like the reference: randperm at :269 and :311):
//   pc_global [B, Lg, 3]            Lg = min(M, 2048)
//   pc_scale[i] [B, M_i, 3], i < 3  the cloud seen by scale i (M_0 = M, then M_i = M_{i-1} // ds_factor)
constexpr int OCC_CHUNK = 16384;
// per-query feature row: [ local 3x256 | x-embedding 512 | view harmonics 64 ] = 1344   (cat at SconeOcc.py:333
// is (global 512, local 768, x 512, harmonics 64); the per-cloud global part is folded into a row bias)
constexpr int FEAT = 1344;
constexpr size_t OCC_WS_SLACK = 8192 + 2 * 1024, OCC_RAGGED_WS_SLACK = 8192 + 1024;

// ---- what the dense and the ragged entry share: the workspace's front, the side stream, everything behind the local features ----
// The head's scratch over T query rows in G groups (clouds / jobs): the workspace of both entries starts with it, the global
// transformer's scratch follows (local and global paths run concurrently, on two streams: disjoint scratch).
struct OccHead {
    float *feat, *h1, *h2, *gfeat, *gbias;
    void* wplanes;                                        // split weight planes of the largest head layer (reused layer after layer)
    // variant 6 with all three fused transformers: the head runs on fp16 hi/lo planes end to end (run_head_planes); the feature
    // buffer then holds planes [2][T][1344] fp16 instead of fp32 [T][1344]
    HeadScratch planes() const { return HeadScratch{reinterpret_cast<_Float16*>(feat), reinterpret_cast<_Float16*>(h1), h2, wplanes}; }
};
static OccHead carve_occ_head(Arena& a, int64_t T, int64_t G) {
    OccHead w;
    w.feat = a.f(T * FEAT);
    w.h1 = a.f(T * 512);
    w.h2 = a.f(T * 256);
    w.gfeat = a.f(G * 512);
    w.gbias = a.f(G * 512);
    w.wplanes = a.bytes(linear3h_planes_bytes(512, 1344));
    return w;
}

// The global feature (a chain of ~20 small launches on 2048 tokens, ~0.3 ms of mostly latency) depends on nothing the local
// path produces and is needed only by the first head layer: it runs on a side stream beside the kNN / local-transformer
// launches (fork / join by events, so a captured graph keeps the structure).  MCR_OCC_OVERLAP=0 puts it back on the caller's stream.
struct OccSide { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
// One side stream + fork / join event pair per (device, CALLER stream): two host streams (or threads) running SconeOcc
// concurrently never share an event pair; creation is serialised.
// slot 0: the global transformer / the cloud build; slot 1: the x embedding queued with the early part (its own stream: on slot 0 the
// cloud build of the first search would queue up behind its GEMMs)
static OccSide* occ_side(hipStream_t caller, int slot = 0) {
    static const bool on = []() { const char* e = getenv("MCR_OCC_OVERLAP"); return !(e && e[0] == '0'); }();
    if (!on) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<std::pair<int, int>, hipStream_t>, OccSide> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    OccSide& x = table[std::make_pair(std::make_pair(dev, slot), caller)];
    if (!x.s) {
        if (hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess) {
            x.s = nullptr;
            return nullptr;
        }
    }
    return &x;
}
// fork the side stream off s: the stream the side work goes to -- s itself, and side = NULL, when there is none or the fork failed
static hipStream_t fork_side(hipStream_t s, OccSide*& side) {
    if (side && hipEventRecord(side->fork, s) == hipSuccess && hipStreamWaitEvent(side->s, side->fork, 0) == hipSuccess) return side->s;
    side = nullptr;
    return s;
}
// every way out of an entry joins the side stream again (error returns included: a dangling fork would poison a capture and
// let side-stream work outlive the caller's workspace): the guard exists before anything is queued on the side stream, and on an
// early return it records the join itself
struct SideJoin {
    OccSide* side; hipStream_t s; bool recorded = false, joined = false;
    ~SideJoin() {
        if (!side || joined) return;
        if (!recorded) (void)hipEventRecord(side->join, side->s);
        (void)hipStreamWaitEvent(s, side->join, 0);
    }
};

// the global feature of G clouds (SconeOcc.py:269-277) and its contribution to linear1: gbias[b, n] = sum_k gfeat[b, k] * W1[n, k]
// (columns 0..511 of linear1.weight)
static void run_global(hipStream_t gs, const OccW& w, const float* pc_global, int64_t G, int64_t Lg, const int* lens, const EncScratch& glob,
                       const OccHead& hd) {
    run_pct(gs, w.global, pc_global, hd.gfeat, 512, G, (int)Lg, 256, glob, lens);
    launch_linear(gs, {hd.gfeat, 512}, {w.lin1.w, 1856}, {nullptr, ACT_NONE}, {hd.gbias, 512}, G, 512, 512, /*route_rows=*/1);
}

// The large layers of the fp32-input head run on the matrix path of the selected variant -- 6: fp16 x 3 with the weights split once
// per call into `wplanes`; 5: bf16 x 6 (exact hi/mid/lo); 1: exact fp32 MFMA -- chosen by the variant and the layer alone, never by
// the number of rows: a query's occupancy must not depend on how many other queries share the launch (query shards of the
// multi-GPU step, chunks, scene batches and the single call agree bit for bit).
// which: as for head_weight_planes (variants 6 / 7).  lin: the layer, its weight rows ldw floats apart
// rb (optional): the row bias, grouped by rows_per_group (dense: rows of one cloud) or by row_group (ragged: the job of each row)
static void head_linear(hipStream_t s, int which, Rows X, const LinW& lin, int64_t ldw, RowsOut Y, int64_t M, int N, int K, RowBias rb,
                        const void* const* head_planes, const float* head_inv_scales, void* wplanes) {
    const int variant = g_local_pct_variant;
    const int64_t ANY_M = (int64_t)1 << 40;
    const Rows W{lin.w, ldw};
    const Epilogue e{lin.b, ACT_GELU, {}, rb};
    if ((variant == 6 || variant == 7) && linear3h_applicable(X.p, X.ld, W.p, W.ld, ANY_M, N, K))
        launch_linear3h(s, X, head_weight_planes(s, which, lin, ldw, N, K, head_planes, head_inv_scales, wplanes), e, Y, M, N, K);
    else if (variant == 5 && linear3_applicable(X.p, X.ld, W.p, W.ld, ANY_M, N, K))
        launch_linear3(s, X, W, e, Y, M, N, K);
    else
        launch_linear(s, X, W, e, Y, M, N, K, /*route_rows=*/1);
}

// Everything behind the local features: x embedding, the join with the side stream (the global feature is needed from the first
// head layer on), head MLP, range guard.  planes: on fp16 planes end to end (x_done: its x embedding has been queued elsewhere).
static int run_occ_head(const char* who, hipStream_t s, const OccW& w, const float* x, const float* view_harmonics, int64_t T, const OccHead& hd,
                        int64_t rows_per_group, const int* row_group, const void* const* head_planes, const float* head_inv_scales, bool planes,
                        bool x_done, OccSide* side, SideJoin& side_join, int* range_flag, float* out) {
    bool join_failed = false;
    auto join = [&]() {
        if (side) {
            side_join.joined = true;
            join_failed = hipStreamWaitEvent(s, side->join, 0) != hipSuccess;
        }
    };
    if (planes)
        run_head_planes(s, x, view_harmonics, T, w.xe1, w.xe2, w.xe3, w.lin1, w.lin2, w.lin3, hd.gbias, rows_per_group, row_group, head_planes,
                        head_inv_scales, hd.planes(), out, join, x_done);
    else {
        // ---- x embedding 3 -> 128 -> 256 -> 512, GELU each (SconeOcc.py:35-42) ----
        launch_linear(s, {x, 3}, {w.xe1.w, 3}, {w.xe1.b, ACT_GELU}, {hd.h2, 128}, T, 128, 3, /*route_rows=*/1);
        head_linear(s, 0, {hd.h2, 128}, w.xe2, 128, {hd.h1, 256}, T, 256, 128, {}, head_planes, head_inv_scales, hd.wplanes);
        head_linear(s, 1, {hd.h1, 256}, w.xe3, 256, {hd.feat + 768, FEAT}, T, 512, 256, {}, head_planes, head_inv_scales, hd.wplanes);
        launch_copy2d(s, view_harmonics, 64, hd.feat + 1280, FEAT, T, 64);
        // ---- head MLP 1856 -> 512 -> 256 -> 1, GELU after every layer incl. the last (SconeOcc.py:334-345) ----
        join();
        MCR_REQUIRE(!join_failed, "%s: side stream (join)", who);
        head_linear(s, 2, {hd.feat, FEAT}, {w.lin1.w + 512, w.lin1.b}, 1856, {hd.h1, 512}, T, 512, FEAT, {hd.gbias, rows_per_group, row_group},
                    head_planes, head_inv_scales, hd.wplanes);
        head_linear(s, 3, {hd.h1, 512}, w.lin2, 512, {hd.h2, 256}, T, 256, 512, {}, head_planes, head_inv_scales, hd.wplanes);
        launch_linear(s, {hd.h2, 256}, {w.lin3.w, 256}, {w.lin3.b, ACT_GELU}, {out, 1}, T, 1, 256, /*route_rows=*/1);
    }
    MCR_REQUIRE(!join_failed, "%s: side stream (join)", who);
    // range guard of the fp16 split path: an activation beyond the fp16 range (|x| >= 65520) becomes inf in its high plane and
    // reaches the output as a non-finite occupancy (inf - inf in the accumulators, NaN through LayerNorm / soft-max / the mean
    // pooling); the caller re-runs on the full-range variant 5 when the flag comes back set
    if (range_flag) launch_nonfinite_flag(s, out, T, range_flag);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

// ---- the dense entry's workspace: head | grid kNN | global transformer | scratch ----
// `scratch` is what is left behind the rest; every (cloud, scale) launch of the local path carves it anew: the [rows,16,3] offsets
// of its queries (only the offsets are consumed, SconeOcc.py:297-298: indices and distances are not written) and, on the
// layer-by-layer path through HBM, the transformer's scratch over rows sequences of 16 points
struct OccLocal { float* offs; EncScratch pct; };
static OccLocal carve_occ_local(Arena& a, int64_t rows, bool layer_by_layer) {
    OccLocal w{};
    w.offs = a.f(rows * 16 * 3);
    if (layer_by_layer) w.pct = carve_enc(a, rows * 16, PCT_E);
    return w;
}
struct OccScratch {
    OccHead head;
    // grid-pruned kNN (knn.hip: K1-grid): the query order of all clouds + one sorted candidate copy per scale (the largest admissible cloud)
    char *knn_q, *knn_c, *knn_park;
    size_t knn_c_bytes;
    EncScratch glob;
    Arena scratch;
};
static OccScratch carve_occ(Arena& a, int64_t B, int64_t Q, int64_t Lg) {
    OccScratch w;
    w.head = carve_occ_head(a, B * Q, B);
    w.knn_c_bytes = knn_grid_cloud_bytes(B, 16384);
    w.knn_q = (char*)a.bytes(knn_grid_query_bytes(B, Q));
    w.knn_c = (char*)a.bytes(3 * w.knn_c_bytes);
    w.knn_park = (char*)a.bytes(knn_grid_park_bytes());
    w.glob = carve_enc(a, B * Lg, PCT_E);
    w.scratch = a.rest();
    return w;
}
size_t mcr_scone_occ_workspace_bytes(int64_t B, int64_t Q, int64_t Lg) {
    // this function knows neither the variant nor whether the fused blobs are given, so `scratch` covers the largest of the forms a
    // call of these dimensions can take: the offsets of all B x Q rows (fused path, a batch of clouds in one launch), one cloud's
    // (fused path, per cloud), or the layer-by-layer path over a chunk of queries
    const size_t local = std::max({measure(carve_occ_local, B * Q, false), measure(carve_occ_local, Q, false),
                                   measure(carve_occ_local, std::min<int64_t>(Q, OCC_CHUNK), true)});
    return measure(carve_occ, B, Q, Lg) + local + OCC_WS_SLACK;
}

int mcr_knn_points(const float* X, const float* pc, int64_t* idx, float* dists, float* pts, int64_t B, int64_t Q, int64_t M,
                   int k, int subtract_query, void* stream);

// mcr_scone_occ_forward (phase 0: the single call, below) or the same in two calls on one stream and ONE workspace.  Phase 1 = what needs neither the view harmonics nor any hidden draw: the
// query order of the grid search, scale 0 (the whole cloud: search + local transformer) -- it reads x, pc_scale[0] and M_scale[0..2]
// only (the sizes of the down-sampled clouds are known before they are drawn) and is the first long kernel of an NBV step, so a
// caller queues it BEFORE it builds the view state, the harmonics and the down-sampled clouds: the host work of those hides behind
// it instead of leaving the GPU idle at the start of the step.  Phase 2 = the rest (global transformer, scales 1 and 2, x
// embedding, head).  phase 0 = both, in the single-call order.
int mcr_scone_occ_forward_phase(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale,
                                const float* x, const float* view_harmonics, float* out, int64_t B, int64_t Q,
                                const float* const* weights, int n_weights, const float* const* local_blobs,
                                const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                size_t workspace_bytes, int phase, void* stream) {
    const char* who = "mcr_scone_occ_forward";
    VariantScope variant_scope_;
    MCR_REQUIRE(phase >= 0 && phase <= 2, "mcr_scone_occ_forward: phase must be 0, 1 or 2");
    const bool early = phase != 2, late = phase != 1;
    MCR_REQUIRE(pc_scale && M_scale && x && weights && (!late || (pc_global && view_harmonics && out)), "mcr_scone_occ_forward: null pointer");
    MCR_REQUIRE(!head_planes || head_inv_scales, "mcr_scone_occ_forward: head_planes need head_inv_scales");
    if (check_table(who, OCC_TABLE, weights, n_weights, n_weights)) return 1;
    MCR_REQUIRE(B > 0 && Q > 0 && Lg > 0 && B <= 65535, "mcr_scone_occ_forward: bad problem size");
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_occ_workspace_bytes(B, Q, Lg), "mcr_scone_occ_forward: workspace too small");
    for (int i = 0; i < 3; ++i)
        MCR_REQUIRE((pc_scale[i] || (!late && i > 0)) && M_scale[i] >= 16, "mcr_scone_occ_forward: scale %d has %ld points (< k = 16)", i,
                    (long)M_scale[i]);
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, n_weights);
    Arena arena{(char*)workspace, workspace_bytes};
    const OccScratch ws = carve_occ(arena, B, Q, Lg);
    MCR_REQUIRE(arena.ok(), "mcr_scone_occ_forward: workspace overflow (global)");
    const OccHead& hd = ws.head;
    float* feat = hd.feat;

    // ---- global feature (SconeOcc.py:269-277), on the side stream ----
    OccSide* side = late ? occ_side(s) : nullptr;
    const hipStream_t gs = fork_side(s, side);
    SideJoin side_join{side, s};
    // fused path: one kNN + one LDS-resident transformer launch per (cloud, scale) over ALL queries (nothing but
    // the [Q,16,3] offsets is materialised); layer-by-layer path: chunked over queries to bound its workspace.
    const bool fused_all = local_blobs && local_blobs[0] && local_blobs[1] && local_blobs[2];
    const int64_t qc = fused_all ? Q : std::min<int64_t>(Q, OCC_CHUNK);
    // the planes head (OccHead::planes); without all three fused blobs, or on variants 1 and 5: the fp32-input head (head_linear)
    const bool planes = fused_all && fp16_planes_variant();
    const int64_t Tall = B * Q;
    const Planes featP = planes_over(hd.feat, Tall, FEAT);
    // The x embedding of the planes head (0.3 ms of GEMMs that need nothing but the queries) has two placements.  Where its own side
    // stream (slot 1) exists it is queued there with the EARLY part (phase 1 / the start of the single call), where the GPU is nearly
    // idle for ~0.4 ms (query order, cloud build, the scale-0 search; profiles/r04_nbv_step_breakdown.txt), and the view harmonics
    // (known in phase 2 only) are split into their columns beside the global transformer.  Otherwise (no stream: creation failed,
    // MCR_OCC_OVERLAP=0) the whole of it runs inside run_head_planes on the caller's stream.
    OccSide* xside = planes ? occ_side(s, 1) : nullptr;   // (the same answer in phase 1 and in phase 2 of one forward)
    // the caller's stream waits for the early x embedding BEHIND the early part's own kernels (end of phase 1 / before the head); every
    // way out of the function in between queues that wait too (a dangling fork would poison a capture)
    struct XJoin {
        OccSide* side; hipStream_t s; bool armed;
        bool wait() { if (!armed) return true; armed = false; return hipStreamWaitEvent(s, side->join, 0) == hipSuccess; }
        ~XJoin() { (void)wait(); }
    } x_join{xside, s, false};
    if (xside && early) {
        MCR_REQUIRE(hipEventRecord(xside->fork, s) == hipSuccess && hipStreamWaitEvent(xside->s, xside->fork, 0) == hipSuccess,
                    "mcr_scone_occ_forward: side stream (x embedding fork)");
        run_x_embedding_planes(xside->s, x, nullptr, B * Q, w.xe1, w.xe2, w.xe3, head_planes, head_inv_scales, hd.planes());
        MCR_REQUIRE(hipEventRecord(xside->join, xside->s) == hipSuccess, "mcr_scone_occ_forward: side stream (x embedding record)");
        x_join.armed = true;
    }
    if (late) {
        run_global(gs, w, pc_global, B, Lg, nullptr, ws.glob, hd);
        if (xside)
            launch_split_to_planes(gs, {view_harmonics, 64}, featP.cols(1280).keep(matrix_planes()), B * Q, 64);
    }
    if (side) {
        MCR_REQUIRE(hipEventRecord(side->join, side->s) == hipSuccess, "mcr_scone_occ_forward: side stream (record)");
        side_join.recorded = true;
    }
    // ---- local multi-scale neighbourhood features (SconeOcc.py:290-311) ----
    // grid-pruned kNN for the scales it applies to (whole-Q launches only): ONE query order for all three scales
    const int* knn_qperm = nullptr;
    KnnGridCloud knn_clouds[3]{};
    int knn_slot[3] = {-1, -1, -1};
    if (qc == Q) {
        const float* g_pc[3]; int64_t g_M[3]; void* g_ws[3];
        int n_grid = 0;
        for (int sc = 0; sc < 3; ++sc)
            if (knn_grid_applicable(M_scale[sc], 16)) {
                g_pc[n_grid] = pc_scale[sc]; g_M[n_grid] = M_scale[sc]; g_ws[n_grid] = ws.knn_c + n_grid * ws.knn_c_bytes;
                knn_slot[sc] = n_grid++;
            }
        if (n_grid) {
            // the query order belongs to phase 1 (phase 2 finds it where phase 1 left it); every scale's cloud is built in the
            // phase that searches it -- all of them in one launch on the single call
            if (phase == 0) {
                knn_qperm = knn_grid_order_queries(s, x, B, Q, ws.knn_q, ws.knn_park);
                knn_grid_build_clouds(s, n_grid, g_pc, g_M, B, g_ws, knn_clouds);
            } else {
                const int first = early ? 0 : (knn_slot[0] >= 0 ? 1 : 0), count = early ? (knn_slot[0] >= 0 ? 1 : 0) : n_grid - first;
                // phase 1 opens the step on an idle GPU: the cloud build (one workgroup per cloud, 40 us) runs on the side stream beside
                // the five small launches of the query order instead of after them
                OccSide* bside = early && count > 0 ? occ_side(s) : nullptr;
                const hipStream_t bs = fork_side(s, bside);
                knn_grid_build_clouds(bs, count, g_pc + first, g_M + first, B, g_ws + first, knn_clouds + first);
                const bool recorded = !bside || hipEventRecord(bside->join, bside->s) == hipSuccess;
                knn_qperm = knn_grid_order_queries(s, x, B, Q, ws.knn_q, ws.knn_park, /*launch=*/early);
                const bool joined = !bside || hipStreamWaitEvent(s, bside->join, 0) == hipSuccess;        // (waits for a stale record at worst)
                MCR_REQUIRE(recorded && joined, "mcr_scone_occ_forward: side stream (cloud build)");
            }
            MCR_LAUNCH_CHECK("knn grid preparation");
        }
    }
    for (int sc = 0; sc < 3; ++sc) {
        if (sc == 0 ? !early : !late) continue;
        const bool grid_knn = knn_slot[sc] >= 0;
        const KnnGridCloud knn_cloud = grid_knn ? knn_clouds[knn_slot[sc]] : KnnGridCloud{};
        const bool fused = planes || (local_blobs && local_blobs[sc]);      // the fused LDS-resident kernel (local_pct*.hip)
        // a batch of clouds on the fused path (config 3's scene batch): ONE search and ONE transformer launch per scale over all B x Q
        // rows instead of one per cloud -- eight brute-force searches of 256 workgroups each (one wave per SIMD: every wave waits out
        // its own latencies) become one of 2048.  The rows are the same rows: same bits.
        if (B > 1 && qc == Q && fused) {
            Arena a = ws.scratch;
            float* offs = carve_occ_local(a, Tall, false).offs;
            MCR_REQUIRE(a.ok(), "mcr_scone_occ_forward: workspace overflow (kNN)");
            if (grid_knn) {
                launch_knn16_grid(s, x, pc_scale[sc], M_scale[sc], knn_qperm, knn_cloud, 0, B, Q, nullptr, nullptr, offs, true, ws.knn_park, sc);
                MCR_LAUNCH_CHECK("knn_grid_kernel");
            } else if (int e = mcr_knn_points(x, pc_scale[sc], nullptr, nullptr, offs, B, Q, M_scale[sc], 16, 1, stream))
                return e;
            if (planes) run_local_pct(s, offs, nullptr, FEAT, Tall, local_blobs[sc], featP.cols(sc * 256));
            else run_local_pct(s, offs, feat + sc * 256, FEAT, Tall, local_blobs[sc]);
            continue;
        }
        for (int64_t q0 = 0; q0 < Q; q0 += qc) {
            const int64_t nq = std::min<int64_t>(qc, Q - q0);
            for (int64_t b = 0; b < B; ++b) {
                Arena a = ws.scratch;
                const OccLocal loc = carve_occ_local(a, nq, !fused);
                MCR_REQUIRE(a.ok(), fused ? "mcr_scone_occ_forward: workspace overflow (kNN)" : "mcr_scone_occ_forward: workspace overflow (local)");
                float* offs = loc.offs;
                if (grid_knn) {
                    launch_knn16_grid(s, x, pc_scale[sc], M_scale[sc], knn_qperm, knn_cloud, b, 1, Q, nullptr, nullptr, offs, true, ws.knn_park,
                                      (int)(sc * B + b));
                    MCR_LAUNCH_CHECK("knn_grid_kernel");
                } else if (int e = mcr_knn_points(x + (b * Q + q0) * 3, pc_scale[sc] + b * M_scale[sc] * 3, nullptr, nullptr, offs, 1, nq,
                                                  M_scale[sc], 16, 1, stream))
                    return e;
                if (planes)                              // (row b * Q + q0, column sc * 256 of both planes)
                    run_local_pct(s, offs, nullptr, FEAT, nq, local_blobs[sc], featP.cols((b * Q + q0) * FEAT + sc * 256));
                else if (fused)
                    run_local_pct(s, offs, feat + (b * Q + q0) * FEAT + sc * 256, FEAT, nq, local_blobs[sc]);
                else                                      // layer-by-layer path through HBM
                    run_pct(s, w.local[sc], offs, feat + (b * Q + q0) * FEAT + sc * 256, FEAT, nq, 16, 128, loc.pct);
            }
        }
    }
    MCR_REQUIRE(x_join.wait(), "mcr_scone_occ_forward: side stream (x embedding join)");
    if (!late) {
        MCR_LAUNCH_CHECK("mcr_scone_occ_forward (phase 1)");
        return 0;
    }
    return run_occ_head(who, s, w, x, view_harmonics, Tall, hd, Q, nullptr, head_planes, head_inv_scales, planes, /*x_done=*/xside != nullptr, side,
                        side_join, range_flag, out);
}

int mcr_scone_occ_forward(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale,
                          const float* x, const float* view_harmonics, float* out, int64_t B, int64_t Q,
                          const float* const* weights, int n_weights, const float* const* local_blobs,
                          const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                          size_t workspace_bytes, void* stream) {
    return mcr_scone_occ_forward_phase(pc_global, Lg, pc_scale, M_scale, x, view_harmonics, out, B, Q, weights, n_weights, local_blobs,
                                       head_planes, head_inv_scales, range_flag, workspace, workspace_bytes, 0, stream);
}

// ---------------------------------------------------------------------------------------------------------
// Ragged SconeOcc: J independent SconeOcc.forward calls ("jobs": one surface cloud + one chunk of queries each, clouds and
// chunks of different sizes -- the per-cell passes of compute_scene_occupancy_probability_field, macarons_utils.py:1395-1540)
// as ONE launch sequence.  Job j: global cloud pc_global[j] (Lg rows, the first global_len[j] valid), neighbourhood clouds
// pc_scale[s][scale_off[s][j] .. scale_off[s][j+1]), queries = the rows r of x with row_job[r] == j (rows sorted by job).
// knn_blocks: n_blocks x int4 (job, first row, rows <= mcr_knn_rows_per_block(), 0) covering every row once.
// Its workspace: head | global transformer | the offsets of all T rows | the segmented search's split scratch
struct OccRaggedScratch { OccHead head; EncScratch glob; float *offs, *knn_split; };
static OccRaggedScratch carve_occ_ragged(Arena& a, int64_t J, int64_t T, int64_t Lg) {
    OccRaggedScratch w;
    w.head = carve_occ_head(a, T, J);
    w.glob = carve_enc(a, J * Lg, PCT_E);
    w.offs = a.f(T * 16 * 3);
    w.knn_split = a.f(knn16_segmented_split_floats(T));
    return w;
}
size_t mcr_scone_occ_ragged_workspace_bytes(int64_t J, int64_t T, int64_t Lg) { return measure(carve_occ_ragged, J, T, Lg) + OCC_RAGGED_WS_SLACK; }
int mcr_knn_rows_per_block(void) { return knn_rows_per_block(); }

// mcr_scone_occ_forward_ragged (phase 0: the single call, below) or the same in two calls on one stream and ONE workspace: phase 1 = everything that needs none of the hidden random draws (scale 0:
// the whole clouds; the x embedding on the planes path), phase 2 = the rest (global transformer, scales 1 and 2, head).  The host
// makes the draws (~60 us of torch.randperm per job) between the two calls while the GPU works on phase 1.  phase 0 = both.
// Phase 1 reads pc_scale[0], scale_off[0], x, view_harmonics, row_job, knn_blocks, local_blobs[0]; phase 2 everything else too.
int mcr_scone_occ_forward_ragged_phase(const float* pc_global, const int* global_len, int64_t Lg, const float* const* pc_scale,
                                       const int64_t* const* scale_off, const float* x, const float* view_harmonics, const int* row_job,
                                       const int* knn_blocks, int64_t n_blocks, float* out, int64_t J, int64_t T,
                                       const float* const* weights, int n_weights, const float* const* local_blobs,
                                       const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                       size_t workspace_bytes, int phase, void* stream) {
    const char* who = "mcr_scone_occ_forward_ragged";
    VariantScope variant_scope_;
    MCR_REQUIRE(phase >= 0 && phase <= 2, "mcr_scone_occ_forward_ragged: phase must be 0, 1 or 2");
    const bool early = phase != 2, late = phase != 1;
    MCR_REQUIRE(pc_scale && scale_off && x && view_harmonics && row_job && knn_blocks && weights && (!late || (pc_global && global_len && out)),
                "mcr_scone_occ_forward_ragged: null pointer");
    if (check_table(who, OCC_TABLE, weights, n_weights, n_weights)) return 1;
    MCR_REQUIRE(J > 0 && T > 0 && Lg > 0 && J <= 32767 && n_blocks > 0, "mcr_scone_occ_forward_ragged: bad problem size");
    MCR_REQUIRE(local_blobs && local_blobs[0] && local_blobs[1] && local_blobs[2],
                "mcr_scone_occ_forward_ragged: needs the fused local-transformer blobs");
    MCR_REQUIRE(!head_planes || head_inv_scales, "mcr_scone_occ_forward_ragged: head_planes need head_inv_scales");
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_occ_ragged_workspace_bytes(J, T, Lg), "mcr_scone_occ_forward_ragged: workspace too small");
    for (int i = 0; i < (late ? 3 : 1); ++i) MCR_REQUIRE(pc_scale[i] && scale_off[i], "mcr_scone_occ_forward_ragged: scale %d is null", i);
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, n_weights);
    Arena arena{(char*)workspace, workspace_bytes};
    const OccRaggedScratch ws = carve_occ_ragged(arena, J, T, Lg);
    MCR_REQUIRE(arena.ok(), "mcr_scone_occ_forward_ragged: workspace overflow (kNN)");
    const OccHead& hd = ws.head;
    const bool planes = fp16_planes_variant();
    const Planes featP = planes_over(hd.feat, T, FEAT);
    auto local_scale = [&](int sc) {                      // one segmented kNN + one fused transformer launch over ALL rows
        // (the whole clouds of scale 0 are the large ones: a launch with few query blocks cuts every job's candidates into slices of
        // ~2048 for more workgroups; slicing the down-sampled clouds of the coarser scales too -- 512 per slice -- measured no better)
        launch_knn16_segmented(s, x, pc_scale[sc], (const long long*)scale_off[sc], knn_blocks, n_blocks, T, ws.offs, ws.knn_split, sc == 0 ? 2048 : 0);
        if (planes) run_local_pct(s, ws.offs, nullptr, FEAT, T, local_blobs[sc], featP.cols(sc * 256));
        else run_local_pct(s, ws.offs, hd.feat + sc * 256, FEAT, T, local_blobs[sc]);
    };
    if (early) {
        if (planes && phase == 1) run_x_embedding_planes(s, x, view_harmonics, T, w.xe1, w.xe2, w.xe3, head_planes, head_inv_scales, hd.planes());
        local_scale(0);
        if (!late) {
            MCR_LAUNCH_CHECK("mcr_scone_occ_forward_ragged (phase 1)");
            return 0;
        }
    }

    OccSide* side = occ_side(s);
    const hipStream_t gs = fork_side(s, side);
    SideJoin side_join{side, s};
    run_global(gs, w, pc_global, J, Lg, global_len, ws.glob, hd);
    if (side) {
        MCR_REQUIRE(hipEventRecord(side->join, side->s) == hipSuccess, "mcr_scone_occ_forward_ragged: side stream (record)");
        side_join.recorded = true;
    }
    // ---- local features of scales 1 and 2 (scale 0: above) ----
    for (int sc = 1; sc < 3; ++sc) local_scale(sc);
    return run_occ_head(who, s, w, x, view_harmonics, T, hd, 0, row_job, head_planes, head_inv_scales, planes, /*x_done=*/phase == 2, side, side_join,
                        range_flag, out);
}

int mcr_scone_occ_forward_ragged(const float* pc_global, const int* global_len, int64_t Lg, const float* const* pc_scale,
                                 const int64_t* const* scale_off, const float* x, const float* view_harmonics, const int* row_job,
                                 const int* knn_blocks, int64_t n_blocks, float* out, int64_t J, int64_t T,
                                 const float* const* weights, int n_weights, const float* const* local_blobs,
                                 const void* const* head_planes, const float* head_inv_scales, int* range_flag, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return mcr_scone_occ_forward_ragged_phase(pc_global, global_len, Lg, pc_scale, scale_off, x, view_harmonics, row_job, knn_blocks, n_blocks, out,
                                              J, T, weights, n_weights, local_blobs, head_planes, head_inv_scales, range_flag, workspace,
                                              workspace_bytes, 0, stream);
}

}  // extern "C"
