// PCTransformer backward (SconeOcc.py:45-130: SconeOcc's global transformer on one 2048-token sequence per cloud, its three local ones on
// B * Q sequences of 16 tokens): mcr_pc_transformer_backward, same scheme on the same launchers at E = 128.  The encoder's forward and
// backward (vb_encoder_fwd / vb_encoder_bwd) are shared with SconeVis and take the width; the attention kernels are compiled for the
// per-head widths (16, 64) and (8, 32).  Sequences of 16 tokens have a fused attention backward of their own (a16_bwd_kernel: one wave per
// sequence, nothing but d_qkv written) and are processed in chunks of PB_CHUNK16 sequences INSIDE the entry, their weight gradients
// summed in chunk order: the workspace holds one chunk whatever S is.  The tail's pooling has its own backward (pb_pool_bwd_kernel).
// (Numerics and determinism: as stated in scone_vis_bwd.hip, for every entry of the backward sources.)
#include "bwd_kernels.h"

namespace mcr {
namespace {
// a later chunk's weight gradients: one contiguous staging area, cut in table order
struct PbSlots { float* dst[PCT_NW]; int off[PCT_NW + 1]; };
__global__ __launch_bounds__(256) void pb_add_slots_kernel(PbSlots t, const float* __restrict__ stage) {
    const int slot = blockIdx.y, n = t.off[slot + 1] - t.off[slot];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) t.dst[slot][e] += stage[t.off[slot] + e];
}

PbScratch carve_pb(Arena& a, int64_t S, int64_t L, int half) {
    const int64_t Sc = pb_chunk(S, L);
    return carve_pb_chunk(a, Sc, L, half, Sc < S);
}
}  // namespace

void Stage::add(hipStream_t s, int blocks) const {
    PbSlots t;
    std::copy(dst, dst + PCT_NW, t.dst);
    std::copy(off, off + PCT_NW + 1, t.off);
    hipLaunchKernelGGL(pb_add_slots_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, t, base);
}

// An encoder of width E (256: SconeVis, 128: PCTransformer) with VB_H heads: q | k of E / 4 channels, v of E, packed rows of 3 E / 2.
// x_out = Encoder(x) (x_out NULL: the interior for the backward, LSE included).  The boundary pass (x_out given) needs no LSE: it takes
// the forward's exact-fp32 MFMA attention (launch_attention, fp32 P V); so does the interior of 16-token sequences
void vb_encoder_fwd(hipStream_t s, const EncW& w, const float* x, float* x_out, const VbInterior& I, int64_t B, int N, const int* lens, int E) {
    const int64_t T = B * N;
    const int QK = E / 4, W3 = enc_qkv(E).N;
    launch_layernorm(s, x, E, w.n1g, w.n1b, I.h1, E, T, E);
    lin_fwd(s, T, enc_qkv(E), w.qkv, {I.h1, E}, {}, {I.qkv, W3});
    if (x_out || vb_fused16(N, E)) launch_attention(s, {I.qkv, W3}, {I.O, E}, B, N, VB_H, QK, E, lens, AttnSplit{}, /*pv_half=*/false);
    else launch_attn_fwd(s, I.qkv, W3, I.O, E, I.lse, B, N, VB_H, lens, I.part, QK / VB_H);
    lin_fwd(s, T, enc_out(E), w.out, {I.O, E}, {x, E}, {I.xm, E});
    launch_layernorm(s, I.xm, E, w.n2g, w.n2b, I.h2, E, T, E);
    lin_fwd(s, T, enc_ff1(E), w.ff1, {I.h2, E}, {}, {I.z, 2 * E}, {I.g, 2 * E});
    if (x_out) lin_fwd(s, T, enc_ff2(E), w.ff2, {I.g, 2 * E}, {I.xm, E}, {x_out, E});
}

// Backward of one encoder (Attention.py:278-300) whose interior I was rebuilt from its input x.  dw: where the gradients of the encoder's
// ENC_NW table entries go (NULL: none wanted)
void vb_encoder_bwd(hipStream_t s, const EncW& we, float* const* dw, const float* x, const VbInterior& I, const VbGrads& G, int64_t B, int N,
                    const int* lens, int E) {
    const int64_t T = B * N;
    const int QK = E / 4, W3 = enc_qkv(E).N;
    float *dX = G.dX, *dH = G.dH, *dA = G.dA, *dQKV = G.dQKV, *part = G.part;
    const LinCtx c{s, T, G.part, G.wt, dw};
    auto DW = [&](int slot) { return dw ? dw[slot] : nullptr; };
    lin_bwd(c, enc_ff2(E), we.ff2, ENC_FF2, {}, {dX, E}, {I.g, 2 * E}, {dH, 2 * E});
    lin_bwd(c, enc_ff1(E), we.ff1, ENC_FF1, {I.z, 2 * E}, {dH, 2 * E}, {I.h2, E}, {dA, E});
    launch_ln_bwd(s, I.xm, E, we.n2g, dA, E, dX, E, true, DW(ENC_N2G), DW(ENC_N2B), part, T, E);   // norm2 (+ residual)
    lin_bwd(c, enc_out(E), we.out, ENC_OUT, {}, {dX, E}, {I.O, E}, {dA, E});
    if (vb_fused16(N, E)) {
        if (lens) { refuse("vb_encoder_bwd: 16-token sequences take no lens (every key takes part)"); return; }
        launch_attn16_bwd(s, I.qkv, W3, dA, E, dQKV, W3, B);
    }
    else launch_attn_bwd(s, I.qkv, W3, I.O, E, I.lse, dA, E, G.delta, dQKV, W3, B, N, VB_H, lens, I.part, QK / VB_H);
    lin_bwd(c, enc_qkv(E), we.qkv, ENC_QKV, {}, {dQKV, W3}, {I.h1, E}, {dA, E});
    launch_ln_bwd(s, x, E, we.n1g, dA, E, dX, E, true, DW(ENC_N1G), DW(ENC_N1B), part, T, E);   // norm1 (+ residual)
}

// ---- PCTransformer (SconeOcc.py:45-130): E = 128, 2 encoders, 4 heads of widths (8, 32) ---------------------------------------------------
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
    auto gw = [T](LinShape l) { return vb_gradw_floats(T, l.N, l.K); };
    G.part = a.f(std::max({gw(enc_ff1(PB_E)), gw(enc_ff2(PB_E)), gw(enc_qkv(PB_E)), gw(pb_lin0(half)), gw(PB_L2), vb_ln_part_floats(T, PB_E)}));
    G.wt = a.f((size_t)2 * PB_E * PB_E);
    w.stage = a.f(with_stage ? pb_stage_floats(half) : 0);
    return w;
}

// Forward of the fp32 network over one chunk of Sc sequences: boundaries X0..X2, the embedding's pre-activation, the tail up to
// linear0's output ws.y0 (what the pooling reads)
// lens (optional, DEVICE int[Sc]): padded sequences -- the keys of sequence i are its first min(L, max(1, lens[i])) rows
void pb_chunk_forward(hipStream_t s, const PctW& w, const float* pc, int64_t Sc, int L, int half, const PbScratch& ws, const int* lens) {
    const int64_t T = Sc * L;
    float* const* X = ws.X;
    lin_fwd(s, T, PB_L1, w.l1, {pc, 3}, {}, {ws.z1, PB_F}, {ws.g1, PB_F});
    lin_fwd(s, T, PB_L2, w.l2, {ws.g1, PB_F}, {}, {X[0], PB_E});
    launch_copy2d(s, pc, 3, X[0] + PB_F, PB_E, T, 3);
    for (int e = 0; e < PCT_N_ENC; ++e) vb_encoder_fwd(s, w.enc[e], X[e], X[e + 1], ws.I, Sc, L, lens, PB_E);
    launch_layernorm(s, X[PCT_N_ENC], PB_E, w.ng, w.nb, ws.hn, PB_E, T, PB_E);
    lin_fwd(s, T, pb_lin0(half), w.lin0, {ws.hn, PB_E}, {}, {ws.y0, half});
}

// One chunk: Sc sequences from pc / d_feat on; dw = where the table's gradients go (NULL: none), d_pc (optional) this chunk's rows;
// ld_feat: the leading dimension of d_feat (0: 2 * half, dense rows); forward_done: ws still holds pb_chunk_forward's results for this
// very chunk (nothing has written it since), so the forward is not run again; lens: as pb_chunk_forward, the pooling's too (padded
// rows then receive exact zeros from the pooling's backward and hand exact zeros on: nothing of them reaches a gradient)
void pb_chunk_backward(hipStream_t s, const PctW& w, const float* pc, const float* d_feat, int64_t Sc, int L, int half, float* const* dw,
                       float* d_pc, const PbScratch& ws, int64_t ld_feat, bool forward_done, const int* lens) {
    const int64_t T = Sc * L;
    float* const* X = ws.X;
    const VbInterior& I = ws.I;
    const VbGrads& G = ws.G;
    const LinCtx c{s, T, G.part, G.wt, dw};
    auto DW = [&](int slot) { return dw ? dw[slot] : nullptr; };
    if (!forward_done) pb_chunk_forward(s, w, pc, Sc, L, half, ws, lens);
    // ---- tail (SconeOcc.py:119-126), backwards: pooling, linear0, norm
    launch_pool_bwd(s, ws.y0, half, d_feat, ld_feat > 0 ? ld_feat : 2 * half, G.dH, half, Sc, L, half, lens);
    lin_bwd(c, pb_lin0(half), w.lin0, PCT_LIN0, {}, {G.dH, half}, {ws.hn, PB_E}, {G.dA, PB_E});
    launch_ln_bwd(s, X[PCT_N_ENC], PB_E, w.ng, G.dA, PB_E, G.dX, PB_E, false, DW(PCT_NG), DW(PCT_NB), G.part, T, PB_E);
    // ---- encoders, last to first
    for (int e = PCT_N_ENC - 1; e >= 0; --e) {
        vb_encoder_fwd(s, w.enc[e], X[e], nullptr, I, Sc, L, lens, PB_E);
        vb_encoder_bwd(s, w.enc[e], dw ? dw + PCT_ENC + ENC_NW * e : nullptr, X[e], I, G, Sc, L, lens, PB_E);
    }
    // ---- embedding (Attention.py:98-128): [linear2(GELU(linear1(pc))) | pc]; d_pc = the raw columns' gradient + linear1's dX
    lin_bwd(c, PB_L2, w.l2, PCT_L2, {}, {G.dX, PB_E}, {ws.g1, PB_F}, {G.dH, PB_F});
    lin_bwd(c, PB_L1, w.l1, PCT_L1, {ws.z1, PB_F}, {G.dH, PB_F}, {pc, 3});
    if (d_pc) {
        launch_copy2d(s, G.dX + PB_F, PB_E, d_pc, 3, T, 3);
        lin_bwd(c, PB_L1, w.l1, LIN_NO_DW, {}, {G.dH, PB_F}, {}, {d_pc, 3}, /*accumulate=*/true);
    }
}
}  // namespace mcr
using namespace mcr;
extern "C" {
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
    if (check_bwd_workspace(who, workspace, workspace_bytes, mcr_pc_transformer_backward_workspace_bytes(S, L))) return 1;
    if (check_d_weights(who, d_weights, PCT_NW)) return 1;
    MCR_REQUIRE(((uintptr_t)pc | (uintptr_t)d_features) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    if (!d_weights && !d_pc) return 0;
    hipStream_t s = (hipStream_t)stream;
    const PctW w = read_pct(weights);
    const int half = feature_dim / 2;
    Arena a{(char*)workspace, workspace_bytes};
    const PbScratch ws = carve_pb(a, S, L, half);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const int64_t Sc = pb_chunk(S, L);
    float* stage_tab[PCT_NW];                              // (staging only when there are chunks behind the first)
    const Stage stage(Sc < S ? d_weights : nullptr, stage_tab, ws.stage, PCT_NW, [half](int k) { return pb_slot_floats(k, half); });
    for (int64_t s0 = 0; s0 < S; s0 += Sc) {
        const int64_t n = std::min(Sc, S - s0);
        float* const* dw = !d_weights ? nullptr : s0 == 0 ? d_weights : stage_tab;
        pb_chunk_backward(s, w, pc + s0 * L * 3, d_features + s0 * feature_dim, n, (int)L, half, dw, d_pc ? d_pc + s0 * L * 3 : nullptr, ws);
        if (d_weights && s0 > 0) stage.add(s);
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

}  // extern "C"
