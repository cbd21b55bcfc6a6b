// A ResNet basic block without stride or downsample (torchvision's BasicBlock as upstream's feature extractor runs it in `layer1`,
// macarons/networks/ManyDepth.py:33-50), for BatchNorm in eval mode, fused, for gfx950 -- the forward.
//
//   t = ReLU( BN1( conv2d(x, w1 [C,C,3,3]; stride 1, zero padding 1, no bias) ) )     [B,C,H,W], kept in the workspace
//   y = ReLU( BN2( conv2d(t, w2 [C,C,3,3]; stride 1, zero padding 1, no bias) ) + x )
//   BN(z) = fmaf(z, a, b) per channel with a = weight * (1.0f / sqrtf(var + eps)), b = fmaf(-mean, a, bias), in float
//
// Two launches of el_conv_kernel (expansion_layer.h) in its zero-padded mode with the convolution's weight order, on
// v_mfma_f32_16x16x4_f32.  The template has an epilogue parameter (AFFINE) for this: the scale and shift of the BatchNorm, an optional
// residual, ReLU, applied where the other instantiations add their bias and apply ELU -- after the partial sums of a channel split have
// been added in the order of the waves.  The tile is the one el_tile chooses for the expansion layers.  No atomics: two calls give the
// same bits.
#include "basic_block.h"

using namespace mcr;

extern "C" size_t mcr_basic_block_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    if (!bb_sizes_ok(B, C, H, W)) return 0;
    return measure(carve_block, B, C, H, W);
}

extern "C" int mcr_basic_block(const float* x, const float* w1, const float* bn1_weight, const float* bn1_bias, const float* bn1_mean,
                               const float* bn1_var, float eps1, const float* w2, const float* bn2_weight, const float* bn2_bias,
                               const float* bn2_mean, const float* bn2_var, float eps2, float* y, int64_t B, int C, int H, int W,
                               void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_basic_block";
    if (int e = bb_check_sizes(who, B, C, H, W)) return e;
    const BlockOperands p{w1, BnOperand{bn1_weight, bn1_bias, bn1_mean, bn1_var, eps1}, w2, BnOperand{bn2_weight, bn2_bias, bn2_mean, bn2_var, eps2}};
    MCR_REQUIRE(x && y && p.all(), "%s: NULL operand", who);
    MCR_REQUIRE(x != y, "%s: y must not be x", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_basic_block_workspace_bytes(B, C, H, W))) return e;
    Arena arena{(char*)workspace, workspace_bytes};
    const BlockScratch ws = carve_block(arena, B, C, H, W);
    bb_launch((hipStream_t)stream, x, p, ws.t, y, B, C, H, W);
    MCR_LAUNCH_CHECK("el_conv_kernel (basic block)");
    return 0;
}
