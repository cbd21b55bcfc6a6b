// Host parts of mcr_cost_volume_backward under the host sanitizers: the workspace size arithmetic and the whole MCR_REQUIRE chain, reached
// with NULL, short or oversized operands so that every call returns before its first launch (no GPU is touched, none is needed).
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I macarons_amd/csrc -x hip tools/cost_volume_backward_host_check.cpp macarons_amd/csrc/cost_volume_bwd.hip \
//         macarons_amd/csrc/cost_volume.hip macarons_amd/csrc/errors.hip -o cost_volume_backward_host_check && ./cost_volume_backward_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/macarons_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        printf("FAIL %s (last error: %s)\n", what, mcr_last_error());
    }
}

struct Args {
    const float *x, *xa, *cams, *bins, *d_out;
    int64_t stride;
    float *d_x, *d_xa;
    int64_t B;
    int A, C, H, W, Hf, Wf, D;
    float fov;
    void* ws;
    size_t ws_bytes;
};

static int call(const Args& a) {
    return mcr_cost_volume_backward(a.x, a.xa, a.cams, a.bins, a.d_out, a.stride, a.d_x, a.d_xa, a.B, a.A, a.C, a.H, a.W, a.Hf, a.Wf, a.D, a.fov,
                                    a.ws, a.ws_bytes, nullptr);
}

static void refused(Args a, const char* word, const char* what) {
    const int rc = call(a);
    expect(rc != 0 && strstr(mcr_last_error(), word) != nullptr, what);
}

int main() {
    // ---- the size: zero for sizes that are not positive or that the entry refuses, growing with every dimension otherwise ----
    expect(mcr_cost_volume_backward_workspace_bytes(0, 2, 64, 64, 114, 96) == 0, "size, B = 0");
    expect(mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, -1) == 0, "size, D < 0");
    expect(mcr_cost_volume_backward_workspace_bytes(1, 2, 64, INT64_MAX, 114, 96) == 0, "size, Hf = INT64_MAX");
    expect(mcr_cost_volume_backward_workspace_bytes(65535, 65535, 64, 1 << 15, 1 << 15, 1 << 18) == 0, "size, everything large");
    size_t prev = 0;
    for (int64_t D = 1; D <= 200; D += 7) {
        const size_t s = mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, D);
        expect(s > prev && s % 256 == 0, "size grows with D in multiples of 256");
        prev = s;
    }
    const size_t need = mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, 96);
    expect(need >= (size_t)96 * 64 * 114 * (16 + 2 * 4 * 8), "size holds the sign states and the index");

    // ---- the refusals: host memory stands in for the operands, no call gets as far as a launch ----
    static float dummy[16];
    void* ws = aligned_alloc(256, 4096);
    Args ok = {dummy, dummy, dummy, dummy, dummy, 96 * 64 * 114, dummy, dummy, 1, 2, 64, 256, 456, 64, 114, 96, 1.7320508f, ws, need};
    Args a = ok;
    a.x = nullptr, refused(a, "NULL operand", "x = NULL");
    a = ok, a.d_out = nullptr, refused(a, "NULL operand", "d_out = NULL");
    a = ok, a.d_x = nullptr, a.d_xa = nullptr, refused(a, "nothing to do", "both outputs NULL");
    a = ok, a.C = 32, refused(a, "feature channels", "C = 32");
    a = ok, a.B = 0, refused(a, "at least 1", "B = 0");
    a = ok, a.D = 0, refused(a, "at least 1", "D = 0");
    a = ok, a.Hf = 300, refused(a, "Hf <= H", "Hf > H");
    a = ok, a.H = 1, a.Hf = 1, refused(a, "H, W >= 2", "H = 1");
    a = ok, a.H = a.W = a.Hf = a.Wf = 65536, refused(a, "too large", "Hf*Wf beyond int");
    a = ok, a.B = 65536, refused(a, "65535", "B beyond the grid");
    a = ok, a.B = 300, a.A = 300, refused(a, "65535", "B*A beyond the grid");
    a = ok, a.B = 64, a.A = 8, a.H = a.W = a.Hf = a.Wf = 512, refused(a, "corner contributions", "more contributions than the lists index");
    a = ok, a.stride = 96 * 64 * 114 - 1, refused(a, "d_out_batch_stride", "a short batch stride");
    a = ok, a.fov = 0.f, refused(a, "fov_scale", "fov_scale = 0");
    a = ok, a.ws_bytes = need - 1, refused(a, "workspace", "a workspace one byte short");
    a = ok, a.ws = nullptr, refused(a, "workspace", "workspace = NULL");
    a = ok, a.ws = (char*)ws + 8, refused(a, "16-byte aligned", "a misaligned workspace");
    a = ok, a.d_x = nullptr, a.ws_bytes = 0, refused(a, "workspace", "d_x = NULL alone is no refusal; the empty workspace is");
    free(ws);
    printf(failures ? "%d checks failed\n" : "all host checks passed\n", failures);
    return failures != 0;
}
