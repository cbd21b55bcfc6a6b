// SconeVis.forward (SconeVis.py:121-162) composed from the encoders of pct.hip and the gfx950 building blocks (nn_kernels.hip) behind one
// C-ABI entry point (include/macarons_hip.h): E = 256, 3 encoders, 4 heads, view_state_mode "end".  The backward side is scone_vis_bwd.hip.
#include "encoder.h"

namespace mcr {
constexpr int VIS_E = 256, VIS_F = 126;
constexpr size_t VIS_WS_SLACK = 4096;
}  // namespace mcr

using namespace mcr;

extern "C" {

size_t mcr_scone_vis_workspace_bytes(int64_t B, int64_t N) { return measure(carve_enc, B * N, VIS_E) + VIS_WS_SLACK; }

int mcr_scone_vis_forward(const float* pts, const float* view_harmonics, float* out, int64_t B, int64_t N,
                          const float* const* weights, int n_weights, const int* lengths, void* workspace,
                          size_t workspace_bytes, void* stream) {
    VariantScope variant_scope_;
    const Numerics& nm = variant_scope_.numerics();
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
    const bool planes = nm.enc_planes((int)N, VIS_E);
    const int np = nm.matrix_planes();                    // 1 on variant 7: the GEMMs below multiply the high planes alone
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
    for (int e = 0; e < 3; ++e) run_encoder(s, nm, w.enc[e], x, h, qkv, ff, B, (int)N, VIS_E, 4, lengths);   // SconeVis.py:139-140
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
        launch_linear(s, {h, VIS_E}, {fc1.w, VIS_E}, {fc1.b, ACT_GELU}, {ff, VIS_E}, T, 192, VIS_E, nm.seq_route(N));
        launch_copy2d(s, view_harmonics, 64, ff + 192, VIS_E, T, 64);
        launch_linear(s, {ff, VIS_E}, {fc2.w, VIS_E}, {fc2.b, ACT_GELU}, {h, 128}, T, 128, VIS_E, nm.seq_route(N));
        launch_linear(s, {h, 128}, {fc3.w, 128}, {fc3.b, ACT_NONE}, {out, 64}, T, 64, 128, N);
    }
    MCR_LAUNCH_CHECK("mcr_scone_vis_forward");
    return 0;
}

}  // extern "C"
