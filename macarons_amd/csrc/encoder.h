// Host-only: what the forward networks (pct.hip, scone_vis.hip, scone_occ.hip) share -- the encoder and PCTransformer runners of
// pct.hip and the range guard's launcher of fwd_blocks.hip.  Whatever depends on the call's numerics variant takes its Numerics.
#pragma once
#include "nn_kernels.h"
#include "net_layout.h"
#include "numerics.h"

namespace mcr {

// The weight planes of one layer: the host-built ones (`given`, scale 1 / given_inv; one split per parameter version instead of per call)
// when the table has them, else planes split here into `scratch` with the fixed 2^8 scale (|w| < 255).  Np, Kp (optional): the layer
// zero-padded to [2][Np][Kp]; its padded bias then goes behind the planes and replaces *bias_p -- on entry the host-built one.
WPlanes weight_planes(hipStream_t s, const void* given, float given_inv, const LinW& lin, int64_t ldw, int N, int K, void* scratch,
                      int Np = 0, int Kp = 0, const float** bias_p = nullptr);

// x <- Encoder(x)  in place.  x [T, E]; scratch h [T, E], qkv [T, 2*dqk + E], ff [T, 2E]
void run_encoder(hipStream_t s, const Numerics& nm, const EncW& w, float* x, float* h, float* qkv, float* ff, int64_t S, int L, int E, int H,
                 const int* lens = nullptr);

// ---- PCTransformer (SconeOcc.py:45-130): S sequences of L points (pts_dim 3), E = 128, 2 encoders, 4 heads ----
constexpr int PCT_E = 128, PCT_INNER = 125;
// The scratch of a stack of encoders of width E over T tokens (PCTransformer: E = 128; SconeVis: E = 256): the residual stream x and
// the encoder's h [T, E], qkv [T, 2*dqk + E] (dqk = E / 4), ff [T, 2E]
struct EncScratch { float *x, *h, *qkv, *ff; };
EncScratch carve_enc(Arena& a, int64_t T, int E);
// feat[s*ld_feat + 0 : feature_dim] ; feature_dim = 2 * half (max || avg)
// lens (optional, device int per sequence): sequence s consists of its first lens[s] rows (zero-padded batch of clouds of
// different sizes): attention keys and the pooling stop there
void run_pct(hipStream_t s, const Numerics& nm, const PctW& w, const float* pc, float* feat, int64_t ld_feat, int64_t S, int L, int half,
             const EncScratch& ws, const int* lens = nullptr);
// the fused local transformer of the call's variant (local_pct*.hip; each variant has its own blob format)
// P (optional): the features as fp16 planes (row stride ld halves) instead of fp32 rows of feat
void run_local_pct(hipStream_t s, const Numerics& nm, const float* offs, float* feat, int64_t ld, int64_t S, const float* blob, Planes P = Planes{});

// *flag |= 1 if any of x[0..n) is inf / NaN (the flag is the caller's: cleared by the caller, OR'ed here)
void launch_nonfinite_flag(hipStream_t s, const float* x, int64_t n, int* flag);

}  // namespace mcr
