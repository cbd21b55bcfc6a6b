// The expansion layers of the depth decoder (macarons/networks/ManyDepth.py:308-363 ExpansionLayer; expansion5..1 of the decoder, :428-471
// and :514-529), fused, for gfx950 -- the forward.
//
//   u = ELU( conv_transpose2d(x, Wu[Cin,Cmid,3,3], bu; stride 1, padding 1) )      [B,Cmid,h,w]
//   r = nearest(u -> (H,W))                                                         torch's mode='nearest': source = min(floor(dst in/out), in-1), in float
//   c = cat(r, x_add) over channels                                                 x_add [B,Cadd,H,W], or absent (Cadd = 0)
//   y = ELU( conv2d(reflect_pad1(c), Wi[Cout,Cmid+Cadd,3,3], bi) )                  [B,Cout,H,W]
//
// Two launches of ONE kernel template, el_conv_kernel (expansion_layer.h, which the backward shares): a 3 x 3 correlation over a virtual
// input of C0 + C1 channels, bias, ELU.  The first
// launch reads the transposed convolution as what it is, a zero-padded correlation with the kernel flipped and its channel axes
// exchanged (tap (di,dj) of output channel co and input channel ci is Wu[ci,co,2-di,2-dj]), over x, into the workspace.  The second reads
// channels below Cmid from u through the nearest-source index and the others from x_add, both through the reflection index: no
// resized, concatenated or padded tensor exists.  What differs between the two is a table of source offsets per cell of the staged region
// (-1: a zero) that the workgroup builds once, and the order in which the weights are read.
//
// The products run on v_mfma_f32_16x16x4_f32, exact fp32 (a k-ordered fmaf chain), as an implicit GEMM per tap: the A operand is 16 output
// channels x 4 input channels of one tap, the B operand 4 input channels x 16 consecutive pixels of a row of the LDS tile, shifted by the
// tap; D is 16 output channels x 16 pixels.  A workgroup of four waves owns TH rows x 16 NSEG columns of one image and 16 MA output
// channels.  KC input channels at a time the tile with its one-pixel ring and the weights of those channels go to LDS -- the weights in
// upstream's own layouts, rearranged to [output channel][channel][tap] (the transposed convolution's taps flipped) while they are staged,
// so nothing is cached on the host; an output channel's row is 2 mod 32 floats long, which keeps the A reads of a wave on distinct banks (9 is
// odd) and the stores of the convolution's weights lane-linear -- through registers, the next chunk on its way while this one is multiplied.  The four waves divide the rows (WK = 1), or, where the map is so
// small that this would leave compute units idle, the input channels of every chunk (WK = 4: groups of four channels round-robin); every
// wave keeps at least two independent accumulators.  The partial sums of a split are added through LDS in the order of the waves, then
// the bias, then ELU: no atomics, two calls give the same bits.
#include "expansion_layer.h"

using namespace mcr;

extern "C" size_t mcr_expansion_layer_workspace_bytes(int64_t B, int64_t Cmid, int64_t h, int64_t w) {
    if (B < 1 || Cmid < 1 || Cmid > EL_MAX_C || h < 1 || w < 1 || h > 0x7fffffffll || w > 0x7fffffffll || !el_fits(B, Cmid, h, w)) return 0;
    return measure(carve_expansion, B, Cmid, h, w);
}

extern "C" int mcr_expansion_layer(const float* x, const float* x_add, const float* up_weight, const float* up_bias, const float* i_weight,
                                   const float* i_bias, float* y, int64_t B, int Cin, int Cmid, int Cadd, int Cout, int h, int w, int H, int W,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_expansion_layer";
    if (int e = el_check_sizes(who, B, Cin, Cmid, Cadd, Cout, h, w, H, W)) return e;
    MCR_REQUIRE(x && up_weight && up_bias && i_weight && i_bias && y && (Cadd == 0 || x_add), "%s: NULL operand", who);
    if (int e = check_workspace(who, workspace, workspace_bytes, mcr_expansion_layer_workspace_bytes(B, Cmid, h, w))) return e;
    Arena arena{(char*)workspace, workspace_bytes};
    const ElScratch ws = carve_expansion(arena, B, Cmid, h, w);
    const hipStream_t st = (hipStream_t)stream;
    el_launch<true>(st, x, nullptr, up_weight, up_bias, ws.u, B, Cin, 0, h, w, Cmid, h, w);
    MCR_LAUNCH_CHECK("el_conv_kernel (transposed convolution)");
    el_launch<false>(st, ws.u, Cadd ? x_add : nullptr, i_weight, i_bias, y, B, Cmid, Cadd, h, w, Cout, H, W);
    MCR_LAUNCH_CHECK("el_conv_kernel (convolution)");
    return 0;
}
