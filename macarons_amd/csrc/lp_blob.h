// Parameter-blob layout of the fused local transformers (local_pct.hip, local_pct5/6/7.hip), built on the host by
// macarons_amd/networks/packing.py: fifteen matrices, then the vectors.  The variants differ in the K padding of the first
// matrix (K0) and in the floats a weight takes (NUM / DEN: their plane formats); everything else is one layout.
#pragma once

namespace mcr {

// matrices, in order:
//   0 emb1 (N128, K padded to K0)  1 emb2 (N128,K128)
//   per encoder e (base 2 + 6e): qkv (N192,K128)  out (N128,K128)  ff1a ff1b (N128,K128)  ff2a ff2b (N128,K128)
//   14 lin0 (N128,K128)
template <int K0, int NUM, int DEN>
struct LpBlob {
    static constexpr int MAT_K0 = 128 * K0 * NUM / DEN, MAT_128 = 128 * 128 * NUM / DEN, MAT_QKV = 192 * 128 * NUM / DEN;
    // idx: 0 emb1, 1 emb2, 2+6e+{0 qkv,1 out,2 ff1a,3 ff1b,4 ff2a,5 ff2b}, 14 lin0, 15 = the end of the matrices
    __host__ __device__ static constexpr int mat_off(int idx) {
        int off = 0;
        for (int i = 0; i < idx; ++i) {
            const bool is_qkv = (i >= 2 && i < 14 && ((i - 2) % 6) == 0);
            off += i == 0 ? MAT_K0 : (is_qkv ? MAT_QKV : MAT_128);
        }
        return off;
    }
};
// vectors, in order: emb1_b[128] emb2_b[128] | per encoder: qkv_c[192] out_b[128] ff1_c[256] ff2_b[128] | lin0_c[128]
constexpr int LP_VEC_EMB1 = 0, LP_VEC_EMB2 = 128, LP_VEC_ENC0 = 256, LP_VEC_ENC_STRIDE = 192 + 128 + 256 + 128,
              LP_VEC_LIN0 = LP_VEC_ENC0 + 2 * LP_VEC_ENC_STRIDE, LP_VECS_TOTAL = LP_VEC_LIN0 + 128;

}  // namespace mcr
