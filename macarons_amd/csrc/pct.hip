// Encoder.forward and PCTransformer.forward composed from the gfx950 building blocks (nn_kernels.hip), the fused local transformers
// behind one runner, and their C-ABI entry points (include/macarons_hip.h).  The backward side is pct_bwd.hip.
//
// Reference (file:line, upstream tree):
//   macarons/networks/Attention.py:98-128   Embedding.forward      (linear-GELU-linear, optional cloud max, concat x)
//   macarons/networks/Attention.py:278-300  Encoder.forward        (pre-LN MHSA + residual, pre-LN FF + residual)
//   macarons/networks/SconeOcc.py:104-130   PCTransformer.forward
// Only the reference's default architecture hyper-parameters are implemented on the HIP path (every call site
// uses them); the Python host classes refuse other configurations loudly.
// The weight tables the entries read and the arena their workspaces are carved from are described once, in net_layout.h; each
// entry's scratch is a struct with one carve function, which its *_workspace_bytes measures.
#include "encoder.h"

namespace mcr {

WPlanes weight_planes(hipStream_t s, const void* given, float given_inv, const LinW& lin, int64_t ldw, int N, int K, void* scratch, int Np,
                      int Kp, const float** bias_p) {
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
static void run_encoder_planes(hipStream_t s, const Numerics& nm, const EncW& w, float* x, float* h, float* qkv, float* ff, int64_t S, int L,
                               int E, int H, const int* lens) {
    const int64_t T = S * L;
    const int dqk = E / 4, W3 = 2 * dqk + E;
    const bool attn_planes = attention_planes_applicable(H, dqk, E, W3);
    // 1 on variant 7 (with head dims the planes attention covers: the default architectures): the LayerNorms' low plane is neither written nor read
    const int np = attn_planes ? nm.matrix_planes() : 2;
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
        if (!launch_attention(s, {qkv, W3}, {h, E}, S, L, H, dqk, E, lens, {ff, ff_floats, 1}, nm.attn_pv_half(), aP))   // :191-198
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

void run_encoder(hipStream_t s, const Numerics& nm, const EncW& w, float* x, float* h, float* qkv, float* ff, int64_t S, int L, int E, int H,
                 const int* lens) {
    const int64_t T = S * L;
    const int dqk = E / 4, W3 = 2 * dqk + E;
    if (nm.enc_planes(L, E)) {
        run_encoder_planes(s, nm, w, x, h, qkv, ff, S, L, E, H, lens);
        return;
    }
    const int64_t route = nm.seq_route(L);   // every GEMM of the networks routes (fp32 vs split precision) on the rows of ONE sequence, not on T: see launch_linear
    const size_t ff_floats = (size_t)T * 2 * E;
    launch_layernorm(s, x, E, w.n1g, w.n1b, h, E, T, E);                                                   // Attention.py:287
    launch_linear(s, {h, E}, {w.qkv.w, E}, {w.qkv.b, ACT_NONE}, {qkv, W3}, T, W3, E, route);               // :186-188
    launch_attention(s, {qkv, W3}, {h, E}, S, L, H, dqk, E, lens, {ff, ff_floats, 1}, nm.attn_pv_half());  // :191-198 (ff is free here: key-split scratch)
    launch_linear(s, {h, E}, {w.out.w, E}, {w.out.b, ACT_NONE, {x, E}}, {x, E}, T, E, E, route);           // :201-202 + residual :290
    launch_layernorm(s, x, E, w.n2g, w.n2b, h, E, T, E);                                                   // :293
    launch_linear(s, {h, E}, {w.ff1.w, E}, {w.ff1.b, ACT_GELU}, {ff, 2 * E}, T, 2 * E, E, route);          // :232
    launch_linear(s, {ff, 2 * E}, {w.ff2.w, 2 * E}, {w.ff2.b, ACT_NONE, {x, E}}, {x, E}, T, E, 2 * E, route);   // :235 + residual :298
}

EncScratch carve_enc(Arena& a, int64_t T, int E) {
    EncScratch w;
    w.x = a.f(T * E);
    w.h = a.f(T * E);
    w.qkv = a.f(T * (E + E / 2));
    w.ff = a.f(T * 2 * E);
    return w;
}

void run_pct(hipStream_t s, const Numerics& nm, const PctW& w, const float* pc, float* feat, int64_t ld_feat, int64_t S, int L, int half,
             const EncScratch& ws, const int* lens) {
    const int64_t T = S * L;
    float *x = ws.x, *h = ws.h, *qkv = ws.qkv, *ff = ws.ff;
    const bool planes = nm.enc_planes(L, PCT_E) && half % 4 == 0;
    const int np = nm.matrix_planes();                    // 1 on variant 7: the GEMMs below multiply the high planes alone
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
    for (int e = 0; e < 2; ++e) run_encoder(s, nm, w.enc[e], x, h, qkv, ff, S, L, PCT_E, 4, lens);
    if (planes) {                                                                            // SconeOcc.py:119-122 on planes
        launch_layernorm_planes(s, {x, PCT_E}, w.ng, w.nb, hP.keep(np), T, PCT_E);
        const WPlanes W0 = weight_planes(s, w.p_lin0, WSPLIT_INV, w.lin0, PCT_E, half, PCT_E, qkv);
        launch_linear3p(s, hP, W0, {w.lin0.b, ACT_NONE}, {ff, half}, T, half, PCT_E, np);
    } else {
        launch_layernorm(s, x, PCT_E, w.ng, w.nb, h, PCT_E, T, PCT_E);                      // SconeOcc.py:119
        launch_linear(s, {h, PCT_E}, {w.lin0.w, PCT_E}, {w.lin0.b, ACT_NONE}, {ff, half}, T, half, PCT_E, nm.seq_route(L));   // :122
    }
    launch_pool_max_avg(s, ff, half, feat, ld_feat, S, L, half, lens);                       // :124-126
}

void run_local_pct(hipStream_t s, const Numerics& nm, const float* offs, float* feat, int64_t ld, int64_t S, const float* blob, Planes P) {
    if (nm.variant == 1) launch_local_pct(s, offs, feat, ld, S, blob);
    else if (nm.variant == 5) launch_local_pct5(s, offs, feat, ld, S, blob);
#ifdef MCR_DEV_LOCAL_PCT8
    else if (nm.variant == 8) launch_local_pct8(s, offs, feat, ld, S, blob);
#endif
    else if (nm.variant == 7) launch_local_pct7(s, offs, feat, ld, S, blob, P.h);   // ONE plane out when P.h is set
    else launch_local_pct6(s, offs, feat, ld, S, blob, P.h, P.l);       // planes out (variant 6 only) when P.h is set
}

}  // namespace mcr

using namespace mcr;

extern "C" {

int mcr_local_pct_blob_floats(void) { return local_pct_blob_floats(); }
int mcr_local_pct3_blob_floats(void) { return local_pct5_blob_floats(); }
int mcr_local_pct6_blob_floats(void) { return local_pct6_blob_floats(); }
int mcr_local_pct7_blob_floats(void) { return local_pct7_blob_floats(); }

int mcr_local_pct_forward(const float* offsets, float* features, int64_t ld_features, int64_t S, const float* blob,
                          void* stream) {
    VariantScope variant_scope_;
    MCR_REQUIRE(offsets && features && blob, "mcr_local_pct_forward: null pointer");
    MCR_REQUIRE(S > 0 && ld_features >= 256, "mcr_local_pct_forward: bad sizes");
    MCR_REQUIRE((reinterpret_cast<uintptr_t>(blob) & 15) == 0, "mcr_local_pct_forward: blob must be 16-byte aligned");
    run_local_pct((hipStream_t)stream, variant_scope_.numerics(), offsets, features, ld_features, S, blob);
    MCR_LAUNCH_CHECK("mcr_local_pct_forward");
    return 0;
}

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
    run_pct((hipStream_t)stream, variant_scope_.numerics(), w, pc, features, feature_dim, S, (int)L, feature_dim / 2, ws);
    MCR_LAUNCH_CHECK("mcr_pc_transformer_forward");
    return 0;
}

}  // extern "C"
