// Host side of the networks' backward passes for gfx950: what the backward sources share.  The launchers and size functions declared
// here are defined in bwd_blocks.hip, attention_bwd.hip and pct_bwd.hip; scone_vis_bwd.hip, pct_bwd.hip and scone_occ_bwd.hip compose
// them.  Like nn_kernels.h for the forward: no kernel bodies (every kernel lives in an anonymous namespace of its source).
#pragma once
#include "nn_kernels.h"
#include "net_layout.h"
#include <algorithm>
#include <cmath>

namespace mcr {

constexpr int VB_H = 4;                                            // heads of every encoder
constexpr size_t VB_WS_SLACK = 4096, VB_BLOCK_WS_SLACK = 1024;

// ---- bwd_blocks.hip -----------------------------------------------------------------------------------------------------------------
size_t vb_gradw_floats(int64_t M, int N, int K);                   // the slabs of one weight-gradient product (lin_bwd's `part`)
size_t vb_ln_part_floats(int64_t M, int E);
void launch_ln_bwd(hipStream_t s, const float* X, int64_t ldx, const float* gamma, const float* dY, int64_t ldy, float* dX, int64_t ldd,
                   bool accumulate, float* d_gamma, float* d_beta, float* part, int64_t M, int E);
void launch_colmax_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dG, int64_t ldg, float* dX, int64_t ldd, int64_t S, int L,
                       int E, const int* lens);
// lens (optional, DEVICE int[S]): the valid rows of every sequence
void launch_pool_bwd(hipStream_t s, const float* X, int64_t ldx, const float* dY, int64_t ldy, float* dX, int64_t ldd, int64_t S, int L, int E,
                     const int* lens = nullptr);
// One linear layer of shape L (net_layout.h) over T rows, the one way the networks say it.  Forward: Y = X W^T + b (+ R), the fp32 GEMM of
// the forward (launch_linear routed on one row: never the split-precision kernels), then G = GELU(Y) when G.p is given.
void lin_fwd(hipStream_t s, int64_t T, LinShape L, const LinW& w, Rows X, Rows R, RowsOut Y, RowsOut G = {});
// Backward, in this order: dY *= GELU'(Z) in place (Z.p given); dW | db = dY^T [X | 1] into dw[slot + LIN_W | LIN_B] (dw NULL or
// slot == LIN_NO_DW: not wanted; L.K == 0: the bias half alone, the column sums of dY); dX = dY W, or dX += dY W with accumulate (dX.p
// given).  part: vb_gradw_floats(T, N, K) floats; wt: N * K floats (the transposed weight of the dX product).
struct LinCtx { hipStream_t s; int64_t T; float *part, *wt; float* const* dw; };
constexpr int LIN_NO_DW = -1;
void lin_bwd(const LinCtx& c, LinShape L, const LinW& w, int slot, Rows Z, RowsOut dY, Rows X, RowsOut dX = {}, bool accumulate = false);

// ---- attention_bwd.hip ----------------------------------------------------------------------------------------------------------------
// part: ab_part_floats(S, L, H, dq, dv) floats of scratch (none needed when the problem is not split); dq: the per-head q / k width, 16
// (v: 64) or 8 (v: 32)
size_t ab_part_floats(int64_t S, int L, int H, int dq = 16, int dv = 64);
void launch_attn_fwd(hipStream_t s, const float* qkv, int64_t ldq, float* O, int64_t ldo, float* lse, int64_t S, int L, int H, const int* lens,
                     float* part, int dq = 16);
void launch_attn_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* O, int64_t ldo, const float* lse, const float* dO,
                     int64_t lddo, float* delta, float* dqkv, int64_t lddq, int64_t S, int L, int H, const int* lens, float* part, int dq = 16);
// d_qkv of S sequences of 16 tokens, 4 heads of widths (8, 32); rows 16-byte aligned, leading dimensions multiples of 4
void launch_attn16_bwd(hipStream_t s, const float* qkv, int64_t ldq, const float* dO, int64_t lddo, float* dqkv, int64_t lddq, int64_t S);

// ---- pct_bwd.hip: the encoder, the PCTransformer's chunk functions, the staging -----------------------------------------------------------
// the encoder's interior, rebuilt from its input x: what its backward reads
struct VbInterior { float *h1, *qkv, *O, *lse, *xm, *h2, *z, *g, *part; };   // part: the attention's split scratch
// The gradient buffers of an encoder's backward: dX [T, E] holds the gradient of the encoder's output on entry and of its input on return
struct VbGrads { float *dX, *dH, *dA, *dQKV, *delta, *part, *wt; };   // part / wt: weight-gradient slabs, transposed weight (lin_bwd)
// Sequences of 16 tokens at the PCTransformer's widths have a backward of their own (a16_bwd_kernel) that rebuilds the soft-max itself.
inline bool vb_fused16(int N, int E) { return N == 16 && E == 128; }
void vb_encoder_fwd(hipStream_t s, const EncW& w, const float* x, float* x_out, const VbInterior& I, int64_t B, int N, const int* lens, int E);
void vb_encoder_bwd(hipStream_t s, const EncW& we, float* const* dw, const float* x, const VbInterior& I, const VbGrads& G, int64_t B, int N,
                    const int* lens, int E);
// Sequences of 16 tokens arrive by the ten thousand (B * Q neighbourhoods): they are processed in chunks of PB_CHUNK16 sequences, a
// function of (S, L) alone, so the workspace does not grow with S; the chunks' weight gradients are summed in chunk order.
constexpr int64_t PB_CHUNK16 = 2048;
inline int64_t pb_chunk(int64_t S, int64_t L) { return L == 16 ? std::min(S, PB_CHUNK16) : S; }

// The chunks (jobs) behind the first leave their weight gradients in one contiguous staging area, cut in table order, and are added in
// chunk order.  dst_: the n <= PCT_NW destinations, a slice of d_weights (NULL: nothing is staged); tab (optional): the same slice of
// the table the chunk is handed, which receives the staging pointers; base: the area, of floats() floats; slot_floats(k): entry k's.
struct Stage {
    float* dst[PCT_NW] = {};                                       // (dst, off: what pb_add_slots_kernel takes as its PbSlots)
    int off[PCT_NW + 1] = {};
    const float* base = nullptr;
    int n = 0;
    Stage() = default;
    template <class SlotFloats>
    Stage(float* const* dst_, float** tab, float* base_, int n_, SlotFloats slot_floats) : base(base_), n(dst_ ? n_ : 0) {
        for (int k = 0; k < n; ++k) {
            dst[k] = dst_[k];
            off[k + 1] = off[k] + slot_floats(k);
            if (tab) tab[k] = base_ + off[k];
        }
    }
    size_t floats() const { return (size_t)off[n]; }
    void add(hipStream_t s, int blocks = 64) const;                // dst[k][e] += its staged floats: pb_add_slots_kernel on dim3(blocks, n)
};

// The workspace of mcr_pc_transformer_backward: one chunk of Sc sequences (T = Sc * L tokens)
struct PbScratch {
    float* X[PCT_N_ENC + 1];                               // the residual stream at the encoder boundaries
    float *z1, *g1;                                        // the embedding's pre-activation and its GELU
    float *hn, *y0;                                        // tail: final LayerNorm, linear0's output (what the pooling reads)
    VbInterior I;                                          // one encoder's interior (the two share it)
    VbGrads G;
    float* stage;                                          // weight gradients of the chunks behind the first
};
// one chunk of Sc sequences; with_stage: the staging area of the chunks behind the first
PbScratch carve_pb_chunk(Arena& a, int64_t Sc, int64_t L, int half, bool with_stage);
void pb_chunk_forward(hipStream_t s, const PctW& w, const float* pc, int64_t Sc, int L, int half, const PbScratch& ws,
                      const int* lens = nullptr);
void pb_chunk_backward(hipStream_t s, const PctW& w, const float* pc, const float* d_feat, int64_t Sc, int L, int half, float* const* dw,
                       float* d_pc, const PbScratch& ws, int64_t ld_feat = 0, bool forward_done = false, const int* lens = nullptr);

}  // namespace mcr
