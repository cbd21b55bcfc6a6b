// SconeOcc.forward (SconeOcc.py:250-347), dense and ragged, composed from the PCTransformers of pct.hip, the neighbour searches (knn.hip)
// and the gfx950 building blocks (nn_kernels.hip) behind single C-ABI entry points (include/macarons_hip.h).  The backward side is
// scone_occ_bwd.hip.  The host supplies the already down-sampled clouds (it consumes torch's CPU generator exactly like the
// reference: randperm at :269 and :311):
//   pc_global [B, Lg, 3]            Lg = min(M, 2048)
//   pc_scale[i] [B, M_i, 3], i < 3  the cloud seen by scale i (M_0 = M, then M_i = M_{i-1} // ds_factor)
#include "encoder.h"
#include "side_stream.h"
#include "../../include/macarons_hip.h"
#include <algorithm>

namespace mcr {

constexpr int OCC_CHUNK = 16384;
// per-query feature row: [ local 3x256 | x-embedding 512 | view harmonics 64 ] = 1344   (cat at SconeOcc.py:333
// is (global 512, local 768, x 512, harmonics 64); the per-cloud global part is folded into a row bias)
constexpr int FEAT = 1344;
constexpr size_t OCC_WS_SLACK = 8192 + 2 * 1024, OCC_RAGGED_WS_SLACK = 8192 + 1024;

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
static void run_x_embedding_planes(hipStream_t s, const Numerics& nm, const float* x, const float* view_harmonics, int64_t T, const LinW& xe1,
                                   const LinW& xe2, const LinW& xe3, const void* const* head_planes, const float* head_inv_scales,
                                   const HeadScratch& w) {
    const Planes fP = planes_over(w.featP, T, 1344), hP = planes_over(w.h1P, T, 256);
    const Planes x1 = planes_over(w.h2 + T * 128, T, 128);
    const int np = nm.matrix_planes();                   // 1 on variant 7: the low planes below are neither written (GEMM epilogues) nor read
    launch_linear_smallk_planes(s, {x, 3}, xe1.w, xe1.b, ACT_GELU, x1, T, 128, 3, /*Np=*/0);   // (planes directly: no fp32 rows, no split pass)
    const WPlanes W2 = head_weight_planes(s, 0, xe2, 128, 256, 128, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, x1, W2, {xe2.b, ACT_GELU}, hP, T, 256, 128, np);
    const WPlanes W3 = head_weight_planes(s, 1, xe3, 256, 512, 256, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, hP, W3, {xe3.b, ACT_GELU}, fP.cols(768), T, 512, 256, np);
    if (view_harmonics) launch_split_to_planes(s, {view_harmonics, 64}, fP.cols(1280).keep(np), T, 64);   // (NULL: the caller splits them later)
}

// x_done: the x-embedding part has been queued elsewhere (the side stream: the join covers it).  Returns whether the join of the
// global branch was accepted.
static bool run_head_planes(hipStream_t s, const Numerics& nm, const float* x, const float* view_harmonics, int64_t T, const LinW& xe1,
                            const LinW& xe2, const LinW& xe3, const LinW& lin1, const LinW& lin2, const LinW& lin3, const float* gbias,
                            int64_t rows_per_group, const int* row_group, const void* const* head_planes, const float* head_inv_scales,
                            const HeadScratch& w, float* out, SideBranch& global, bool x_done = false) {
    const Planes fP = planes_over(w.featP, T, 1344), hP = planes_over(w.h1P, T, 512);
    const int np = nm.matrix_planes();
    if (!x_done) run_x_embedding_planes(s, nm, x, view_harmonics, T, xe1, xe2, xe3, head_planes, head_inv_scales, w);
    const bool joined = global.join();                    // the global feature (side stream) is needed from here on
    // head MLP 1856 -> 512 -> 256 -> 1, GELU after every layer incl. the last (SconeOcc.py:334-345); the global 512 columns are gbias
    const WPlanes W1 = head_weight_planes(s, 2, {lin1.w + 512, lin1.b}, 1856, 512, 1344, head_planes, head_inv_scales, w.wplanes);
    launch_linear3p(s, fP, W1, {lin1.b, ACT_GELU, {}, {gbias, rows_per_group, row_group}}, hP, T, 512, 1344, np);
    const WPlanes W2 = head_weight_planes(s, 3, lin2, 512, 256, 512, head_planes, head_inv_scales, w.wplanes);
    // 512 -> 256 (GELU) -> 1 (GELU) in one launch: the block owns all 256 features of its rows and dots them with linear3.weight
    launch_linear3p_dot(s, hP, W2, {lin2.b, ACT_GELU}, T, 512, lin3.w, lin3.b, ACT_GELU, out, np);
    return joined;
}

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

// the global feature of G clouds (SconeOcc.py:269-277) and its contribution to linear1: gbias[b, n] = sum_k gfeat[b, k] * W1[n, k]
// (columns 0..511 of linear1.weight)
static void run_global(hipStream_t gs, const Numerics& nm, const OccW& w, const float* pc_global, int64_t G, int64_t Lg, const int* lens,
                       const EncScratch& glob, const OccHead& hd) {
    run_pct(gs, nm, w.global, pc_global, hd.gfeat, 512, G, (int)Lg, 256, glob, lens);
    launch_linear(gs, {hd.gfeat, 512}, {w.lin1.w, 1856}, {nullptr, ACT_NONE}, {hd.gbias, 512}, G, 512, 512, /*route_rows=*/1);
}

// The large layers of the fp32-input head run on the matrix path of the selected variant -- 6: fp16 x 3 with the weights split once
// per call into `wplanes`; 5: bf16 x 6 (exact hi/mid/lo); 1: exact fp32 MFMA -- chosen by the variant and the layer alone, never by
// the number of rows: a query's occupancy must not depend on how many other queries share the launch (query shards of the
// multi-GPU step, chunks, scene batches and the single call agree bit for bit).
// which: as for head_weight_planes (variants 6 / 7).  lin: the layer, its weight rows ldw floats apart
// rb (optional): the row bias, grouped by rows_per_group (dense: rows of one cloud) or by row_group (ragged: the job of each row)
static void head_linear(hipStream_t s, const Numerics& nm, int which, Rows X, const LinW& lin, int64_t ldw, RowsOut Y, int64_t M, int N, int K,
                        RowBias rb, const void* const* head_planes, const float* head_inv_scales, void* wplanes) {
    const int64_t ANY_M = (int64_t)1 << 40;
    const Rows W{lin.w, ldw};
    const Epilogue e{lin.b, ACT_GELU, {}, rb};
    if (nm.planes() && linear3h_applicable(X.p, X.ld, W.p, W.ld, ANY_M, N, K))
        launch_linear3h(s, X, head_weight_planes(s, which, lin, ldw, N, K, head_planes, head_inv_scales, wplanes), e, Y, M, N, K);
    else if (nm.variant == 5 && linear3_applicable(X.p, X.ld, W.p, W.ld, ANY_M, N, K))
        launch_linear3(s, X, W, e, Y, M, N, K);
    else
        launch_linear(s, X, W, e, Y, M, N, K, /*route_rows=*/1);
}

// Everything behind the local features: x embedding, the join of the global branch (the global feature is needed from the first
// head layer on), head MLP, range guard.  planes: on fp16 planes end to end (x_done: its x embedding has been queued elsewhere).
static int run_occ_head(const char* who, hipStream_t s, const Numerics& nm, const OccW& w, const float* x, const float* view_harmonics, int64_t T,
                        const OccHead& hd, int64_t rows_per_group, const int* row_group, const void* const* head_planes,
                        const float* head_inv_scales, bool planes, bool x_done, SideBranch& global, int* range_flag, float* out) {
    if (planes)
        MCR_REQUIRE(run_head_planes(s, nm, x, view_harmonics, T, w.xe1, w.xe2, w.xe3, w.lin1, w.lin2, w.lin3, hd.gbias, rows_per_group, row_group,
                                    head_planes, head_inv_scales, hd.planes(), out, global, x_done),
                    "%s: side stream (join)", who);
    else {
        // ---- x embedding 3 -> 128 -> 256 -> 512, GELU each (SconeOcc.py:35-42) ----
        launch_linear(s, {x, 3}, {w.xe1.w, 3}, {w.xe1.b, ACT_GELU}, {hd.h2, 128}, T, 128, 3, /*route_rows=*/1);
        head_linear(s, nm, 0, {hd.h2, 128}, w.xe2, 128, {hd.h1, 256}, T, 256, 128, {}, head_planes, head_inv_scales, hd.wplanes);
        head_linear(s, nm, 1, {hd.h1, 256}, w.xe3, 256, {hd.feat + 768, FEAT}, T, 512, 256, {}, head_planes, head_inv_scales, hd.wplanes);
        launch_copy2d(s, view_harmonics, 64, hd.feat + 1280, FEAT, T, 64);
        // ---- head MLP 1856 -> 512 -> 256 -> 1, GELU after every layer incl. the last (SconeOcc.py:334-345) ----
        MCR_REQUIRE(global.join(), "%s: side stream (join)", who);
        head_linear(s, nm, 2, {hd.feat, FEAT}, {w.lin1.w + 512, w.lin1.b}, 1856, {hd.h1, 512}, T, 512, FEAT, {hd.gbias, rows_per_group, row_group},
                    head_planes, head_inv_scales, hd.wplanes);
        head_linear(s, nm, 3, {hd.h1, 512}, w.lin2, 512, {hd.h2, 256}, T, 256, 512, {}, head_planes, head_inv_scales, hd.wplanes);
        launch_linear(s, {hd.h2, 256}, {w.lin3.w, 256}, {w.lin3.b, ACT_GELU}, {out, 1}, T, 1, 256, /*route_rows=*/1);
    }
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

}  // namespace mcr

using namespace mcr;

extern "C" {

size_t mcr_scone_occ_workspace_bytes(int64_t B, int64_t Q, int64_t Lg) {
    // this function knows neither the variant nor whether the fused blobs are given, so `scratch` covers the largest of the forms a
    // call of these dimensions can take: the offsets of all B x Q rows (fused path, a batch of clouds in one launch), one cloud's
    // (fused path, per cloud), or the layer-by-layer path over a chunk of queries
    const size_t local = std::max({measure(carve_occ_local, B * Q, false), measure(carve_occ_local, Q, false),
                                   measure(carve_occ_local, std::min<int64_t>(Q, OCC_CHUNK), true)});
    return measure(carve_occ, B, Q, Lg) + local + OCC_WS_SLACK;
}

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
    const Numerics& nm = variant_scope_.numerics();
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

    // ---- global feature (SconeOcc.py:269-277), on the side stream (a failed fork: on the caller's) ----
    SideBranch global(s, late ? occ_side(s) : nullptr);
    // fused path: one kNN + one LDS-resident transformer launch per (cloud, scale) over ALL queries (nothing but
    // the [Q,16,3] offsets is materialised); layer-by-layer path: chunked over queries to bound its workspace.
    const bool fused_all = local_blobs && local_blobs[0] && local_blobs[1] && local_blobs[2];
    const int64_t qc = fused_all ? Q : std::min<int64_t>(Q, OCC_CHUNK);
    // the planes head (OccHead::planes); without all three fused blobs, or on variants 1 and 5: the fp32-input head (head_linear)
    const bool planes = fused_all && nm.planes();
    const int64_t Tall = B * Q;
    const Planes featP = planes_over(hd.feat, Tall, FEAT);
    // The x embedding of the planes head (0.3 ms of GEMMs that need nothing but the queries) has two placements.  Where its own side
    // stream (slot 1) exists it is queued there with the EARLY part (phase 1 / the start of the single call), where the GPU is nearly
    // idle for ~0.4 ms (query order, cloud build, the scale-0 search; profiles/r04_nbv_step_breakdown.txt), and the view harmonics
    // (known in phase 2 only) are split into their columns beside the global transformer.  Otherwise (no stream: creation failed,
    // MCR_OCC_OVERLAP=0) the whole of it runs inside run_head_planes on the caller's stream.
    OccSide* xside = planes ? occ_side(s, 1) : nullptr;   // (the same answer in phase 1 and in phase 2 of one forward)
    // the caller's stream waits for the early x embedding BEHIND the early part's own kernels (end of phase 1 / before the head); every
    // way out of the function in between queues that wait too
    SideBranch x_early(s, early ? xside : nullptr);
    if (xside && early) {
        MCR_REQUIRE(x_early.forked(), "mcr_scone_occ_forward: side stream (x embedding fork)");
        run_x_embedding_planes(x_early.stream(), nm, x, nullptr, B * Q, w.xe1, w.xe2, w.xe3, head_planes, head_inv_scales, hd.planes());
        MCR_REQUIRE(x_early.record(), "mcr_scone_occ_forward: side stream (x embedding record)");
    }
    if (late) {
        run_global(global.stream(), nm, w, pc_global, B, Lg, nullptr, ws.glob, hd);
        if (xside)
            launch_split_to_planes(global.stream(), {view_harmonics, 64}, featP.cols(1280).keep(nm.matrix_planes()), B * Q, 64);
    }
    MCR_REQUIRE(global.record(), "mcr_scone_occ_forward: side stream (record)");
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
                // the five small launches of the query order instead of after them (a failed fork: in front of them)
                SideBranch build(s, early && count > 0 ? occ_side(s) : nullptr);
                knn_grid_build_clouds(build.stream(), count, g_pc + first, g_M + first, B, g_ws + first, knn_clouds + first);
                const bool recorded = build.record();
                knn_qperm = knn_grid_order_queries(s, x, B, Q, ws.knn_q, ws.knn_park, /*launch=*/early);
                const bool joined = build.join();                                                          // (waits for a stale record at worst)
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
            if (planes) run_local_pct(s, nm, offs, nullptr, FEAT, Tall, local_blobs[sc], featP.cols(sc * 256));
            else run_local_pct(s, nm, offs, feat + sc * 256, FEAT, Tall, local_blobs[sc]);
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
                    run_local_pct(s, nm, offs, nullptr, FEAT, nq, local_blobs[sc], featP.cols((b * Q + q0) * FEAT + sc * 256));
                else if (fused)
                    run_local_pct(s, nm, offs, feat + (b * Q + q0) * FEAT + sc * 256, FEAT, nq, local_blobs[sc]);
                else                                      // layer-by-layer path through HBM
                    run_pct(s, nm, w.local[sc], offs, feat + (b * Q + q0) * FEAT + sc * 256, FEAT, nq, 16, 128, loc.pct);
            }
        }
    }
    MCR_REQUIRE(x_early.join(), "mcr_scone_occ_forward: side stream (x embedding join)");
    if (!late) {
        MCR_LAUNCH_CHECK("mcr_scone_occ_forward (phase 1)");
        return 0;
    }
    return run_occ_head(who, s, nm, w, x, view_harmonics, Tall, hd, Q, nullptr, head_planes, head_inv_scales, planes, /*x_done=*/xside != nullptr,
                        global, range_flag, out);
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
    const Numerics& nm = variant_scope_.numerics();
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
    const bool planes = nm.planes();
    const Planes featP = planes_over(hd.feat, T, FEAT);
    auto local_scale = [&](int sc) {                      // one segmented kNN + one fused transformer launch over ALL rows
        // (the whole clouds of scale 0 are the large ones: a launch with few query blocks cuts every job's candidates into slices of
        // ~2048 for more workgroups; slicing the down-sampled clouds of the coarser scales too -- 512 per slice -- measured no better)
        launch_knn16_segmented(s, x, pc_scale[sc], (const long long*)scale_off[sc], knn_blocks, n_blocks, T, ws.offs, ws.knn_split, sc == 0 ? 2048 : 0);
        if (planes) run_local_pct(s, nm, ws.offs, nullptr, FEAT, T, local_blobs[sc], featP.cols(sc * 256));
        else run_local_pct(s, nm, ws.offs, hd.feat + sc * 256, FEAT, T, local_blobs[sc]);
    };
    if (early) {
        if (planes && phase == 1) run_x_embedding_planes(s, nm, x, view_harmonics, T, w.xe1, w.xe2, w.xe3, head_planes, head_inv_scales, hd.planes());
        local_scale(0);
        if (!late) {
            MCR_LAUNCH_CHECK("mcr_scone_occ_forward_ragged (phase 1)");
            return 0;
        }
    }

    SideBranch global(s, occ_side(s));                    // the global feature, on the side stream (a failed fork: on the caller's)
    run_global(global.stream(), nm, w, pc_global, J, Lg, global_len, ws.glob, hd);
    MCR_REQUIRE(global.record(), "mcr_scone_occ_forward_ragged: side stream (record)");
    // ---- local features of scales 1 and 2 (scale 0: above) ----
    for (int sc = 1; sc < 3; ++sc) local_scale(sc);
    return run_occ_head(who, s, nm, w, x, view_harmonics, T, hd, 0, row_job, head_planes, head_inv_scales, planes, /*x_done=*/phase == 2, global,
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
