// Host-only: the two data formats the network entry points (pct.hip, scone_vis.hip, scone_occ.hip; the backwards: scone_vis_bwd.hip, pct_bwd.hip,
// scone_occ_bwd.hip) share with their callers.
//   1. The weight tables (arrays of device pointers; order documented in include/macarons_hip.h, produced by networks/packing.py):
//      slot names, table lengths, the structs the entries work on, ONE reader per struct and ONE validation.  No table index is
//      written as an integer anywhere else.
//   2. The caller's workspace: the bump allocator, its one rounding rule and `measure` live in workspace.h (the depth module carves its
//      workspaces with them too) and come in through this header.  Every entry describes its scratch as a struct of pointers with one carve
//      function next to the code that uses it; its *_workspace_bytes runs that same function on a measuring arena, so the stated size and
//      the layout cannot drift apart, and every carve is checked against the capacity.
#pragma once
#include "workspace.h"

namespace mcr {

// ---- weight tables ---------------------------------------------------------------------------------------------------------------
// Slots (offsets into the table) of each building block, in table order; *_NW = the block's length.
constexpr int LIN_W = 0, LIN_B = 1, LIN_NW = 2;                                                     // nn.Linear: weight, bias
constexpr int ENC_N1G = 0, ENC_N1B = 1, ENC_QKV = 2, ENC_OUT = ENC_QKV + LIN_NW, ENC_N2G = ENC_OUT + LIN_NW, ENC_N2B = ENC_N2G + 1,
              ENC_FF1 = ENC_N2B + 1, ENC_FF2 = ENC_FF1 + LIN_NW, ENC_NW = ENC_FF2 + LIN_NW;         // ENCODER (12)
constexpr int ENC_PLANES_NW = 4;                       // PLANES tail, per encoder: qkv, out, ff1, ff2
constexpr int PCT_N_ENC = 2, PCT_L1 = 0, PCT_L2 = PCT_L1 + LIN_NW, PCT_ENC = PCT_L2 + LIN_NW, PCT_NG = PCT_ENC + PCT_N_ENC * ENC_NW,
              PCT_NB = PCT_NG + 1, PCT_LIN0 = PCT_NB + 1, PCT_NW = PCT_LIN0 + LIN_NW;               // PCT (32)
constexpr int PCT_END_PLANES_NW = 3;                   // END PLANES tail: linear2 planes, its padded bias, linear0 planes
constexpr int VIS_N_ENC = 3, VIS_L1 = 0, VIS_L2 = VIS_L1 + LIN_NW, VIS_ENC = VIS_L2 + LIN_NW, VIS_NG = VIS_ENC + VIS_N_ENC * ENC_NW,
              VIS_NB = VIS_NG + 1, VIS_FC1 = VIS_NB + 1, VIS_FC2 = VIS_FC1 + LIN_NW, VIS_FC3 = VIS_FC2 + LIN_NW,
              VIS_NW = VIS_FC3 + LIN_NW;                                                            // SCONE_VIS (48)
constexpr int VIS_END_PLANES_NW = 5;                   // END PLANES tail: linear2 planes, its padded bias, fc1, fc2, fc3 planes
constexpr int OCC_GLOBAL = 0, OCC_LOCAL = OCC_GLOBAL + PCT_NW, OCC_XE = OCC_LOCAL + 3 * PCT_NW, OCC_LIN = OCC_XE + 3 * LIN_NW,
              OCC_NW = OCC_LIN + 3 * LIN_NW;                                                        // SCONE_OCC (140)
static_assert(ENC_NW == 12 && PCT_NW == 32 && VIS_NW == 48 && OCC_NW == 140, "table lengths of include/macarons_hip.h");

// What a table may look like: n entries, optionally + planes (the encoders' tail), optionally + ends more (the end layers' tail).
struct TableSpec { int n, planes, ends; };
constexpr TableSpec PCT_TABLE{PCT_NW, PCT_N_ENC * ENC_PLANES_NW, PCT_END_PLANES_NW};
constexpr TableSpec VIS_TABLE{VIS_NW, VIS_N_ENC * ENC_PLANES_NW, VIS_END_PLANES_NW};
constexpr TableSpec OCC_TABLE{OCC_NW, PCT_N_ENC * ENC_PLANES_NW, PCT_END_PLANES_NW};                // (the global transformer's tails)

// The one validation of (weights, n_weights): an accepted length, the first n_required entries non-null (the forwards read the
// tails too: n_required = n_weights; the backward accepts and ignores them).  Returns 0, or 1 with the entry's message set.
inline int check_table(const char* who, const TableSpec& t, const float* const* weights, int n_weights, int n_required) {
    MCR_REQUIRE(n_weights == t.n || n_weights == t.n + t.planes || n_weights == t.n + t.planes + t.ends,
                "%s: expected %d weight pointers (+ %d or %d plane pointers), got %d", who, t.n, t.planes, t.planes + t.ends, n_weights);
    for (int i = 0; i < n_required; ++i) MCR_REQUIRE(weights[i], "%s: weight %d is null", who, i);
    return 0;
}
// ... and of a backward's table of gradient destinations: optional as a whole, complete when given
inline int check_d_weights(const char* who, float* const* d_weights, int n) {
    if (d_weights)
        for (int i = 0; i < n; ++i) MCR_REQUIRE(d_weights[i], "%s: d_weights[%d] is null", who, i);
    return 0;
}
inline bool has_planes(const TableSpec& t, int n_weights) { return n_weights >= t.n + t.planes; }
inline bool has_end_planes(const TableSpec& t, int n_weights) { return n_weights == t.n + t.planes + t.ends; }

// nn.Linear as the table holds it: weight [N, K] (N outputs of K inputs), bias [N].  ONE shape per layer: the backwards' forward and
// backward helpers (bwd_kernels.h: lin_fwd / lin_bwd) and the sizes of the table's entries (the staging areas) all read it.
struct LinShape { int N, K; };
constexpr int lin_slot_floats(LinShape l, int slot) { return slot == LIN_W ? l.N * l.K : l.N; }     // slot: LIN_W or LIN_B
// the layers of an encoder of width E: packed q | k | v (q, k of E / 4 channels, v of E), out, ff1, ff2
constexpr LinShape enc_qkv(int E) { return {E / 2 + E, E}; }
constexpr LinShape enc_out(int E) { return {E, E}; }
constexpr LinShape enc_ff1(int E) { return {2 * E, E}; }
constexpr LinShape enc_ff2(int E) { return {E, 2 * E}; }
// floats of the encoder's table entry `slot` (< ENC_NW): its four layers, else a LayerNorm's gamma or beta
constexpr int enc_slot_floats(int slot, int E) {
    return slot >= ENC_FF2 ? lin_slot_floats(enc_ff2(E), slot - ENC_FF2) : slot >= ENC_FF1 ? lin_slot_floats(enc_ff1(E), slot - ENC_FF1)
           : slot >= ENC_N2G ? E : slot >= ENC_OUT ? lin_slot_floats(enc_out(E), slot - ENC_OUT)
           : slot >= ENC_QKV ? lin_slot_floats(enc_qkv(E), slot - ENC_QKV) : E;
}
// the PCTransformer (E = 128): its embedding, its tail (half = feature_dim / 2); floats of its table entry `slot`, and of the whole table
constexpr int PB_E = 128, PB_F = 125, PB_W3 = 2 * 32 + PB_E;        // PB_F: the embedding's inner width (E - 3: the raw points fill the row)
constexpr LinShape PB_L1{PB_F, 3}, PB_L2{PB_F, PB_F};
constexpr LinShape pb_lin0(int half) { return {half, PB_E}; }
static_assert(enc_qkv(PB_E).N == PB_W3, "packed q | k | v width");
constexpr int pb_slot_floats(int slot, int half) {
    return slot >= PCT_LIN0 ? lin_slot_floats(pb_lin0(half), slot - PCT_LIN0) : slot >= PCT_NG ? PB_E                        // (the final norm)
           : slot >= PCT_ENC ? enc_slot_floats((slot - PCT_ENC) % ENC_NW, PB_E) : lin_slot_floats(slot >= PCT_L2 ? PB_L2 : PB_L1, slot % LIN_NW);
}
inline size_t pb_stage_floats(int half) {
    size_t n = 0;
    for (int i = 0; i < PCT_NW; ++i) n += pb_slot_floats(i, half);
    return n;
}

struct LinW { const float* w; const float* b; };
struct EncW {
    const float *n1g, *n1b;         // norm1
    LinW qkv;                       // rows of w_q, w_k, w_v stacked: [2*dqk + dv, E]
    LinW out;
    const float *n2g, *n2b;         // norm2
    LinW ff1, ff2;
    // optional (NULL: split per call): the four weight matrices as fp16 hi/lo planes [2][N][K] of W * 2^8, built by the host once per
    // parameter version (networks/packing.py: encoder_weight_planes) -- pointers 4 per encoder appended to the weight table
    const void *p_qkv = nullptr, *p_out = nullptr, *p_ff1 = nullptr, *p_ff2 = nullptr;
};
struct PctW { LinW l1, l2; EncW enc[PCT_N_ENC]; const float *ng, *nb; LinW lin0;
              const void *p_l2 = nullptr; const float* b_l2p = nullptr; const void* p_lin0 = nullptr; };   // host-built planes of the end layers (optional)
struct VisW { LinW l1, l2; EncW enc[VIS_N_ENC]; const float *ng, *nb; LinW fc1, fc2, fc3;
              const void *p_l2 = nullptr; const float* b_l2p = nullptr; const void *p_fc1 = nullptr, *p_fc2 = nullptr, *p_fc3 = nullptr; };   // (the same)
struct OccW { PctW global, local[3]; LinW xe1, xe2, xe3, lin1, lin2, lin3; };

inline LinW read_lin(const float* const* p) { return {p[LIN_W], p[LIN_B]}; }
inline EncW read_enc(const float* const* p) {
    EncW e;
    e.n1g = p[ENC_N1G]; e.n1b = p[ENC_N1B];
    e.qkv = read_lin(p + ENC_QKV); e.out = read_lin(p + ENC_OUT);
    e.n2g = p[ENC_N2G]; e.n2b = p[ENC_N2B];
    e.ff1 = read_lin(p + ENC_FF1); e.ff2 = read_lin(p + ENC_FF2);
    return e;
}
// the PLANES tail of n_enc encoders; returns the tail's end
inline const float* const* read_enc_planes(const float* const* p, EncW* enc, int n_enc) {
    for (int e = 0; e < n_enc; ++e) { enc[e].p_qkv = *p++; enc[e].p_out = *p++; enc[e].p_ff1 = *p++; enc[e].p_ff2 = *p++; }
    return p;
}
inline PctW read_pct(const float* const* p) {
    PctW w;
    w.l1 = read_lin(p + PCT_L1); w.l2 = read_lin(p + PCT_L2);
    for (int e = 0; e < PCT_N_ENC; ++e) w.enc[e] = read_enc(p + PCT_ENC + e * ENC_NW);
    w.ng = p[PCT_NG]; w.nb = p[PCT_NB];
    w.lin0 = read_lin(p + PCT_LIN0);
    return w;
}
// the optional tails behind table `t` (n_weights entries in all): they belong to one PCT, w
inline void read_pct_tails(PctW& w, const TableSpec& t, const float* const* weights, int n_weights) {
    const float* const* p = weights + t.n;
    if (has_planes(t, n_weights)) p = read_enc_planes(p, w.enc, PCT_N_ENC);
    if (has_end_planes(t, n_weights)) { w.p_l2 = *p++; w.b_l2p = *p++; w.p_lin0 = *p++; }
}
inline VisW read_vis_table(const float* const* weights, int n_weights) {
    const float* const* p = weights;
    VisW w;
    w.l1 = read_lin(p + VIS_L1); w.l2 = read_lin(p + VIS_L2);
    for (int e = 0; e < VIS_N_ENC; ++e) w.enc[e] = read_enc(p + VIS_ENC + e * ENC_NW);
    w.ng = p[VIS_NG]; w.nb = p[VIS_NB];
    w.fc1 = read_lin(p + VIS_FC1); w.fc2 = read_lin(p + VIS_FC2); w.fc3 = read_lin(p + VIS_FC3);
    p += VIS_NW;
    if (has_planes(VIS_TABLE, n_weights)) p = read_enc_planes(p, w.enc, VIS_N_ENC);
    if (has_end_planes(VIS_TABLE, n_weights)) { w.p_l2 = *p++; w.b_l2p = *p++; w.p_fc1 = *p++; w.p_fc2 = *p++; w.p_fc3 = *p++; }
    return w;
}
inline OccW read_occ_table(const float* const* weights, int n_weights) {
    OccW w;
    w.global = read_pct(weights + OCC_GLOBAL);
    read_pct_tails(w.global, OCC_TABLE, weights, n_weights);                             // the tails are the global transformer's
    for (int i = 0; i < 3; ++i) w.local[i] = read_pct(weights + OCC_LOCAL + i * PCT_NW);
    const float* const* xe = weights + OCC_XE;
    w.xe1 = read_lin(xe); w.xe2 = read_lin(xe + LIN_NW); w.xe3 = read_lin(xe + 2 * LIN_NW);
    const float* const* lin = weights + OCC_LIN;
    w.lin1 = read_lin(lin); w.lin2 = read_lin(lin + LIN_NW); w.lin3 = read_lin(lin + 2 * LIN_NW);
    return w;
}

}  // namespace mcr
