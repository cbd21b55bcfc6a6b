// Device geometry the depth module's kernels share: the pose of a source camera relative to the target and the ray of a full-resolution
// pixel.  The projection of a point along that ray is NOT here, on purpose: the plane sweep (cost_volume.h) projects in fp32 with one fma
// per tap, the reconstruction loss (reconstruction_loss.hip) in double with the derivative by the depth, and each is pinned by its own
// goldens.  They are two computations, not two copies of one.
#pragma once
#include "common.h"

namespace mcr {

// Column k (0..2) of the pose of source camera `cama` seen from target camera `cam0` (12 floats each: R row-major, then T), into out[12]
// doubles: M = R^T R_a (row-major) and t = T_a - T M, so that the source-view point of the target-view point v is v M + t.
__device__ __forceinline__ void pose_column(const float* cam0, const float* cama, int k, double* out) {
    double tk = (double)cama[9 + k];
    for (int jj = 0; jj < 3; ++jj) {
        const double mjk = (double)cam0[jj] * (double)cama[k] + (double)cam0[3 + jj] * (double)cama[3 + k] +
                           (double)cam0[6 + jj] * (double)cama[6 + k];
        out[3 * jj + k] = mjk;
        tk -= (double)cam0[9 + jj] * mjk;
    }
    out[9 + k] = tk;
}

// The ray per unit depth of pixel (row p, column q) of an H x W image is (nx, ny, 1), m = min(H, W).
__device__ __forceinline__ void pixel_ray(int H, int W, float fov_scale, int p, int q, double& nx, double& ny) {
    const int m = min(H, W);
    const double s = (double)fov_scale;
    nx = ((double)W / m - 2.0 * q / (m - 1)) / s, ny = ((double)H / m - 2.0 * p / (m - 1)) / s;
}

}  // namespace mcr
