// Shared device/host helpers for the MI355X (gfx950, wave64) kernels of the SCONE coverage-gain path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MCR_WAVE 64

namespace mcr {

// ---- error plumbing (C-ABI returns int; message kept per thread) -----------------------------------
void set_error(const char* fmt, ...);
// A launcher (void: it sits inside chains of launches) that cannot run its call says so here and returns without launching; the
// entry point's next MCR_LAUNCH_CHECK then returns 3 with this message, whatever hipGetLastError() holds.
void refuse(const char* fmt, ...);
int check_hip(hipError_t e, const char* what);

#define MCR_REQUIRE(cond, ...)                       \
    do {                                             \
        if (!(cond)) {                               \
            ::mcr::set_error(__VA_ARGS__);           \
            return 1;                                \
        }                                            \
    } while (0)

#define MCR_LAUNCH_CHECK(name)                                           \
    do {                                                                 \
        if (int _e = ::mcr::check_hip(hipGetLastError(), name)) return _e; \
    } while (0)

__host__ __device__ static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Chunk c of `chunks` equal chunks of [0, n): [i0, i1), empty past the end.
__device__ __forceinline__ void chunk_range(int64_t n, int chunks, int c, int64_t& i0, int64_t& i1) {
    const int64_t per = cdiv(n, chunks);
    i0 = c * per, i1 = min(n, i0 + per);
}

}  // namespace mcr

#include "wave.h"   // wave and workgroup reductions, scans, the arg-max ordering
