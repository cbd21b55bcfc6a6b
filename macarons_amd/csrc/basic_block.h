// What the basic-block entry (basic_block.hip) and the whole feature extractor (resnet_stem.hip) share: the operands of one ResNet basic
// block, its size checks, its scratch and its two launches of el_conv_kernel (expansion_layer.h) with the affine epilogue.
#pragma once
#include "expansion_layer.h"

namespace mcr {

// An eval-mode BatchNorm: torch's four vectors [C] and eps.
struct BnOperand {
    const float *weight, *bias, *mean, *var;
    float eps;
    bool all() const { return weight && bias && mean && var; }
};

struct BlockOperands {
    const float* w1;   // conv1.weight [C,C,3,3]
    BnOperand bn1;
    const float* w2;   // conv2.weight [C,C,3,3]
    BnOperand bn2;
    bool all() const { return w1 && w2 && bn1.all() && bn2.all(); }
};

// The order of a block's ten device pointers in mcr_feature_extractor's host array, with its two eps.
static BlockOperands block_operands(const float* const* p, const float* eps) {
    return BlockOperands{p[0], BnOperand{p[1], p[2], p[3], p[4], eps[0]}, p[5], BnOperand{p[6], p[7], p[8], p[9], eps[1]}};
}

static bool bb_sizes_ok(int64_t B, int64_t C, int64_t H, int64_t W) {
    return B >= 1 && C >= 1 && C <= EL_MAX_C && H >= 1 && W >= 1 && H <= 0x7fffffffll && W <= 0x7fffffffll && el_fits(B, C, H, W);
}

static int bb_check_sizes(const char* who, int64_t B, int C, int H, int W) {
    MCR_REQUIRE(H >= 1 && W >= 1, "%s: the map is %d x %d, H and W must be at least 1", who, H, W);
    MCR_REQUIRE(C >= 1 && C <= EL_MAX_C, "%s: C = %d channels, 1 .. %d are supported", who, C, EL_MAX_C);
    MCR_REQUIRE(B >= 1, "%s: B = %lld must be at least 1", who, (long long)B);
    MCR_REQUIRE(bb_sizes_ok(B, C, H, W), "%s: B = %lld, %d channels, %d x %d: a tensor has 2^31 elements or more", who, (long long)B, C, H, W);
    return 0;
}

struct BlockScratch { float* t; };                     // [B,C,H,W]: the first convolution after its BatchNorm and ReLU
static BlockScratch carve_block(Arena& a, int64_t B, int64_t C, int64_t H, int64_t W) {
    BlockScratch s;
    s.t = a.f((size_t)(B * C * H * W));
    return s;
}

// relu(BatchNorm(conv3x3(src, weight [C,C,3,3]; stride 1, zero padding 1)) + residual) over [B,C,H,W], on the tile el_tile chooses
static void el_launch_affine(hipStream_t st, const float* src, const float* weight, float* out, int64_t B, int C, int H, int W,
                             const ElAffine& epi) {
    switch (el_tile(B, C, H, W)) {
        case EL_ROWS16: el_launch_as<false, 0, 4, 2, 1, 1, 16, true>(st, src, nullptr, weight, nullptr, out, B, C, 0, H, W, C, H, W, epi); break;
        case EL_ROWS32: el_launch_as<false, 0, 4, 2, 2, 1, 16, true>(st, src, nullptr, weight, nullptr, out, B, C, 0, H, W, C, H, W, epi); break;
        case EL_SPLIT: el_launch_as<false, 0, 2, 1, 1, 4, 32, true>(st, src, nullptr, weight, nullptr, out, B, C, 0, H, W, C, H, W, epi); break;
    }
}

// t = relu(bn1(conv(x, w1))), y = relu(bn2(conv(t, w2)) + x); y must not be x (a workgroup reads x's ring while others store y).
static void bb_launch(hipStream_t st, const float* x, const BlockOperands& p, float* t, float* y, int64_t B, int C, int H, int W) {
    el_launch_affine(st, x, p.w1, t, B, C, H, W, ElAffine{p.bn1.weight, p.bn1.bias, p.bn1.mean, p.bn1.var, nullptr, p.bn1.eps});
    el_launch_affine(st, t, p.w2, y, B, C, H, W, ElAffine{p.bn2.weight, p.bn2.bias, p.bn2.mean, p.bn2.var, x, p.bn2.eps});
}

}  // namespace mcr
