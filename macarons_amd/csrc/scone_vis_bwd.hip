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
// Building blocks (each behind its own C entry point, include/macarons_hip.h): attention (attention_bwd.hip); linear, layernorm,
// column max (bwd_blocks.hip); the encoder (pct_bwd.hip).
// Numerics: fp32 throughout -- VALU FMA in the attention and weight-gradient kernels, the forward's exact-fp32 GEMM kernels
// (launch_linear routed to the fp32 MFMA kernel) in the recompute and the dX products.  The fp16 planes path is never taken, whatever the caller's variant: the result is the gradient of
// the fp32 network at the given inputs (on variants 6 and 7 too).  No float atomics: two calls give identical bits.
#include "bwd_kernels.h"

namespace mcr {
namespace {
// ---- the network -------------------------------------------------------------------------------------------------------------------
// (the weight table and the arena of the workspace: net_layout.h)
constexpr int VB_E = 256, VB_F = 126;
constexpr int VB_W3 = 2 * 64 + VB_E;                             // packed q | k | v width
constexpr LinShape VB_L1{VB_F, 4}, VB_L2{VB_F, VB_F}, VB_FC1{192, VB_E}, VB_FC2{128, VB_E}, VB_FC3{64, 128};   // embedding, head
static_assert(enc_qkv(VB_E).N == VB_W3 && VB_FC1.N + 64 == VB_FC2.K && VB_FC2.N == VB_FC3.K, "SconeVis layout");

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
    w.hn = a.f(T * VB_E); w.zf1 = a.f(T * VB_FC1.N); w.c2 = a.f(T * VB_E); w.zf2 = a.f(T * VB_FC2.N); w.gf2 = a.f(T * VB_FC2.N);
    VbInterior& I = w.I;
    I.h1 = a.f(T * VB_E); I.qkv = a.f(T * VB_W3); I.O = a.f(T * VB_E); I.lse = a.f(T * VB_H);
    I.xm = a.f(T * VB_E); I.h2 = a.f(T * VB_E); I.z = a.f(T * 2 * VB_E); I.g = a.f(T * 2 * VB_E);
    w.dX = a.f(T * VB_E); w.dH = a.f(T * 2 * VB_E); w.dA = a.f(T * VB_E); w.dQKV = a.f(T * VB_W3); w.delta = a.f(T * VB_H);
    auto gw = [T](LinShape l) { return vb_gradw_floats(T, l.N, l.K); };              // (the encoder's layers are the largest)
    w.part = a.f(std::max({gw(enc_ff1(VB_E)), gw(enc_ff2(VB_E)), gw(enc_qkv(VB_E)), vb_ln_part_floats(T, VB_E)}));
    w.wt = a.f((size_t)2 * VB_E * VB_E);
    I.part = a.f(ab_part_floats(B, (int)N, VB_H));
    return w;
}
}  // namespace
}  // namespace mcr
using namespace mcr;
extern "C" {
size_t mcr_scone_vis_backward_workspace_bytes(int64_t B, int64_t N) { return (B > 0 && N > 0) ? measure(carve_vb, B, N) + VB_WS_SLACK : 0; }

int mcr_scone_vis_backward(const float* pts, const float* view_harmonics, const float* d_out, int64_t B, int64_t N, const float* const* weights,
                           int n_weights, const int* lengths, float* const* d_weights, float* d_pts, float* d_view_harmonics, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_vis_backward";
    MCR_REQUIRE(pts && view_harmonics && d_out && weights, "%s: null pointer", who);
    if (check_table(who, VIS_TABLE, weights, n_weights, VIS_NW)) return 1;                  // (a planes tail is accepted and ignored)
    MCR_REQUIRE(B > 0 && N > 0 && B <= 65535 && N <= (1 << 24), "%s: bad problem size B=%ld N=%ld", who, (long)B, (long)N);
    MCR_REQUIRE(workspace && workspace_bytes >= mcr_scone_vis_backward_workspace_bytes(B, N), "%s: workspace too small", who);
    if (check_d_weights(who, d_weights, VIS_NW)) return 1;
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
    const LinCtx c{s, T, part, wt, d_weights};

    // ---- forward of the fp32 network: boundaries X0..X3, the embedding's and the head's pre-activations
    lin_fwd(s, T, VB_L1, w.l1, {pts, 4}, {}, {z1, VB_F}, {g1, VB_F});
    lin_fwd(s, T, VB_L2, w.l2, {g1, VB_F}, {}, {X[0], VB_E});
    launch_colmax_broadcast(s, X[0], VB_E, X[0] + VB_F, VB_E, B, iN, VB_F, lengths, pts, 4, 4, X[0] + 2 * VB_F);
    for (int e = 0; e < 3; ++e) vb_encoder_fwd(s, w.enc[e], X[e], X[e + 1], I, B, iN, lengths, VB_E);
    launch_layernorm(s, X[3], VB_E, w.ng, w.nb, hn, VB_E, T, VB_E);
    lin_fwd(s, T, VB_FC1, w.fc1, {hn, VB_E}, {}, {zf1, 192}, {c2, VB_E});
    launch_copy2d(s, view_harmonics, 64, c2 + 192, VB_E, T, 64);
    lin_fwd(s, T, VB_FC2, w.fc2, {c2, VB_E}, {}, {zf2, 128}, {gf2, 128});

    // ---- head (SconeVis.py:143-152), backwards: fc3, fc2, then fc1 behind the harmonics' columns
    lin_bwd(c, VB_FC3, w.fc3, VIS_FC3, {}, {const_cast<float*>(d_out), 64}, {gf2, 128}, {dH, 128});    // (no GELU: d_out is only read)
    lin_bwd(c, VB_FC2, w.fc2, VIS_FC2, {zf2, 128}, {dH, 128}, {c2, VB_E}, {dA, VB_E});
    if (d_view_harmonics) launch_copy2d(s, dA + 192, VB_E, d_view_harmonics, 64, T, 64);
    if (!d_weights && !d_pts) { MCR_LAUNCH_CHECK(who); return 0; }
    lin_bwd(c, VB_FC1, w.fc1, VIS_FC1, {zf1, 192}, {dA, VB_E}, {hn, VB_E}, {dH, VB_E});
    launch_ln_bwd(s, X[3], VB_E, w.ng, dH, VB_E, dX, VB_E, false, DW(VIS_NG), DW(VIS_NB), part, T, VB_E);   // norm

    // ---- encoders (Attention.py:278-300), last to first; dX holds the gradient of the encoder's output
    const VbGrads G{dX, dH, dA, dQKV, delta, part, wt};
    for (int e = 2; e >= 0; --e) {
        const int o = VIS_ENC + ENC_NW * e;                               // the encoder's block of the table
        vb_encoder_fwd(s, w.enc[e], X[e], nullptr, I, B, iN, lengths, VB_E);              // the interior, from the boundary
        vb_encoder_bwd(s, w.enc[e], d_weights ? d_weights + o : nullptr, X[e], I, G, B, iN, lengths, VB_E);
    }

    // ---- embedding (Attention.py:98-128): [res | cloud max of res | pts]; d_pts = the raw columns' gradient + linear1's dX
    launch_colmax_bwd(s, X[0], VB_E, dX + VB_F, VB_E, dX, VB_E, B, iN, VB_F, lengths);
    lin_bwd(c, VB_L2, w.l2, VIS_L2, {}, {dX, VB_E}, {g1, VB_F}, {dH, VB_F});
    lin_bwd(c, VB_L1, w.l1, VIS_L1, {z1, VB_F}, {dH, VB_F}, {pts, 4});
    if (d_pts) {
        launch_copy2d(s, dX + 2 * VB_F, VB_E, d_pts, 4, T, 4);
        lin_bwd(c, VB_L1, w.l1, LIN_NO_DW, {}, {dH, VB_F}, {}, {d_pts, 4}, /*accumulate=*/true);
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

}  // extern "C"
