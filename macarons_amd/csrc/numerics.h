// Host-only: the numerics variant of ONE network call, as a value.
// 1: local_pct.hip exact-fp32 MFMA; 5: local_pct5.hip split-precision bf16 hi/mid/lo (6 MFMAs per product, whole fp32
// range); 6 (default): local_pct6.hip two-term fp16 split (3 MFMAs per product); 7 (OPT-IN, per call only -- never a process
// default): local_pct7.hip, ONE fp16 plane per matrix operand (1 MFMA per product), BASELINE.json config 3's 16-bit matrix
// path with its own stated tolerance (tests/test_variant7_gpu.py).  Each has its own blob format.
#pragma once
#include "common.h"

namespace mcr {

#ifdef MCR_DEV_LOCAL_PCT8      // dev builds only (tools/build_variant.py with tools/experiments/local_pct8.hip): the shelved register-resident kernel as variant 8
void launch_local_pct8(hipStream_t s, const float* offs, float* feat, int64_t ld_feat, int64_t S, const float* blob);
#define MCR_VARIANT8_OK(v) ((v) == 8)
#else
#define MCR_VARIANT8_OK(v) false
#endif

// What a network call's variant decides; fixed when the entry opens its VariantScope.  Whatever depends on the variant takes one of
// these: no function outside numerics.hip reads thread-local or global variant state.
struct Numerics {
    int variant;                  // 1, 5, 6, 7 (8 in MCR_DEV_LOCAL_PCT8 builds)
    // Variant 7 shares variant 6's routes (operands as fp16 planes in HBM, the same range guard); what differs is how many planes a
    // product multiplies: matrix_planes() = 1 on variant 7 (the high planes alone; low planes are neither written nor read where
    // the single-plane kernels exist: the local transformers and the SconeOcc head), 2 on variant 6.
    bool planes() const { return variant == 6 || variant == 7; }
    int matrix_planes() const { return variant == 7 ? 1 : 2; }
    // rows-per-sequence argument of launch_linear for the encoders of the 2048-token networks (SconeVis, SconeOcc's global
    // transformer): on the split-precision variants (5, 6) their GEMMs take the split-precision kernel for EVERY launch size (negative
    // argument = "choose on the layer's shape"; its column-tile width follows the launch, which does not change a single bit) -- one
    // sequence costs the same as on the fp32 kernels, 8 or 30 sequences in one launch (scene batch, the neighbour cameras of a MACARONS
    // decision) run 1.3x faster, and a sequence's result still does not depend on how many share the launch.  Variant 1 = exact fp32
    // everywhere.  The wide layers behind the encoders (SconeVis fc1 / fc2, the global transformer's lin0) take the same route.
    int64_t seq_route(int64_t L) const { return variant >= 5 ? -L : L; }
    // long-sequence attention: P V on fp16 hi/lo pairs (nn_kernels.hip: PVH) on the fp16-split variants, fp32 MFMA on the others
    bool attn_pv_half() const { return planes(); }
    // Encoder GEMMs of the long-sequence networks on fp16 hi/lo PLANES (variants 6 and 7, sequences of >= 512 tokens; shorter ones take the
    // bf16 x 6 kernels as on variant 5): the GEMM inputs are split once where they are produced -- LayerNorm writes planes, the FF's
    // first GEMM writes planes, the attention output is split in one pass -- and every operand reaches LDS by DMA (linear3p.hip): no
    // split and no staging registers inside the GEMMs, three MFMAs per product instead of six.  Chosen on the sequence length alone, so a
    // cloud's result does not depend on how many clouds share the launch.  Needs |activation| < 65504 like the rest of variant 6: the
    // occupancy / harmonics that come out non-finite otherwise are what the range guards look at.  The layers either side of the encoders
    // (the embeddings' second layer, the final LayerNorm and the fc / lin0 layers behind it) are on the same path under the same condition.
    bool enc_planes(int L, int E) const { return planes() && L >= 512 && E % 32 == 0; }
};

// The variant is a property of a CALL, not of the process: a network entry point opens a VariantScope as its first statement, which fixes
// the call's numerics -- the one-shot value mcr_call_variant(v) left for it on this thread (the per-call argument of the ABI: "the next
// network entry point on this thread runs on v"), else the process default (mcr_set_local_pct_variant / env MCR_LOCAL_PCT_VARIANT).
// The constructor consumes the one-shot, so it runs before any MCR_REQUIRE: a call that fails validation leaves no one-shot behind.
// Two host threads, or two models on different variants, cannot see each other's choice.  No scoped entry calls another one.
class VariantScope {
    const Numerics nm_;
public:
    VariantScope();
    VariantScope(const VariantScope&) = delete;
    const Numerics& numerics() const { return nm_; }
};

}  // namespace mcr
