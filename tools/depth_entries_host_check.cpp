// Host parts of the six depth-module entries (cost volume, reconstruction loss, disparity scales; forward and backward) under the host
// sanitizers: the workspace carve arithmetic behind every *_workspace_bytes and the whole check chain of every entry, reached with NULL,
// short, misaligned or oversized operands so that every call returns before its first launch (no GPU is touched, none is needed).
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I macarons_amd/csrc -x hip tools/depth_entries_host_check.cpp macarons_amd/csrc/cost_volume.hip macarons_amd/csrc/cost_volume_bwd.hip \
//         macarons_amd/csrc/reconstruction_loss.hip macarons_amd/csrc/disparity_scales.hip macarons_amd/csrc/errors.hip \
//         -o depth_entries_host_check && ./depth_entries_host_check
#include <math.h>
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

static void refused(int rc, const char* word, const char* what) { expect(rc != 0 && strstr(mcr_last_error(), word) != nullptr, what); }

static float dummy[16];
static unsigned char dummy_mask[16];
static void* ws;                                     // 4096 bytes of host memory, 256-byte aligned: never reached by a launch

// The three workspace refusals every entry shares: `call(workspace, bytes)` with everything else valid.
template <class Call>
static void workspace_refusals(const char* who, size_t need, Call call) {
    char what[128];
    expect(need > 0 && need % 256 == 0, who);
    snprintf(what, sizeof what, "%s: a workspace one byte short", who), refused(call(ws, need - 1), "workspace", what);
    snprintf(what, sizeof what, "%s: workspace = NULL", who), refused(call(nullptr, need), "workspace", what);
    snprintf(what, sizeof what, "%s: a misaligned workspace", who), refused(call((char*)ws + 8, need + 8), "16-byte aligned", what);
}

// ---- the plane-sweep cost volume, both ways ----
struct CvArgs {
    const float *x, *xa, *cams, *bins, *io;          // io: the forward's out, the backward's d_out
    int64_t stride;
    float *d_x, *d_xa;
    int64_t B;
    int A, C, H, W, Hf, Wf, D;
    float fov;
    void* ws;
    size_t ws_bytes;
};

static int cv_fwd(const CvArgs& a) {
    return mcr_cost_volume(a.x, a.xa, a.cams, a.bins, (float*)a.io, a.stride, a.B, a.A, a.C, a.H, a.W, a.Hf, a.Wf, a.D, a.fov, a.ws, a.ws_bytes,
                           nullptr);
}
static int cv_bwd(const CvArgs& a) {
    return mcr_cost_volume_backward(a.x, a.xa, a.cams, a.bins, a.io, a.stride, a.d_x, a.d_xa, a.B, a.A, a.C, a.H, a.W, a.Hf, a.Wf, a.D, a.fov,
                                    a.ws, a.ws_bytes, nullptr);
}

static void cost_volume_checks() {
    // the sizes: zero for sizes that are not positive or that the entry refuses, growing with every dimension otherwise
    expect(mcr_cost_volume_workspace_bytes(0, 2, 64, 64, 114) == 0, "cv size, B = 0");
    expect(mcr_cost_volume_workspace_bytes(1, 2, 64, 64, -114) == 0, "cv size, Wf < 0");
    expect(mcr_cost_volume_backward_workspace_bytes(0, 2, 64, 64, 114, 96) == 0, "cv bwd size, B = 0");
    expect(mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, -1) == 0, "cv bwd size, D < 0");
    expect(mcr_cost_volume_backward_workspace_bytes(1, 2, 64, INT64_MAX, 114, 96) == 0, "cv bwd size, Hf = INT64_MAX");
    expect(mcr_cost_volume_backward_workspace_bytes(65535, 65535, 64, 1 << 15, 1 << 15, 1 << 18) == 0, "cv bwd size, everything large");
    size_t prev = 0;
    for (int64_t D = 1; D <= 200; D += 7) {
        const size_t s = mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, D);
        expect(s > prev && s % 256 == 0, "cv bwd size grows with D in multiples of 256");
        prev = s;
    }
    // the forward's size is the unrounded sum of its two blocks, rounded up: never less, at most 2 * 255 more (odd sizes: B*A*12 doubles
    // and an odd P are no multiples of 256)
    for (int64_t Wf = 1; Wf <= 9; ++Wf) {
        const size_t raw = (size_t)3 * 1 * (64 * 5 * Wf * sizeof(float) + 12 * sizeof(double)), s = mcr_cost_volume_workspace_bytes(3, 1, 64, 5, Wf);
        expect(s >= raw && s < raw + 512 && s % 256 == 0, "cv size is the sum of its blocks, rounded up");
    }
    const size_t need_f = mcr_cost_volume_workspace_bytes(1, 2, 64, 64, 114), need_b = mcr_cost_volume_backward_workspace_bytes(1, 2, 64, 64, 114, 96);
    expect(need_b >= (size_t)96 * 64 * 114 * (16 + 2 * 4 * 8), "cv bwd size holds the sign states and the index");

    // the refusals: host memory stands in for the operands, no call gets as far as a launch
    const CvArgs ok_f = {dummy, dummy, dummy, dummy, dummy, 96 * 64 * 114, nullptr, nullptr, 1, 2, 64, 256, 456, 64, 114, 96, 1.7320508f, ws, need_f};
    CvArgs ok_b = ok_f;
    ok_b.d_x = ok_b.d_xa = dummy, ok_b.ws_bytes = need_b;
    struct { const char* who; const CvArgs& ok; int (*call)(const CvArgs&); } both[] = {{"cv", ok_f, cv_fwd}, {"cv bwd", ok_b, cv_bwd}};
    for (const auto& e : both) {
        CvArgs a = e.ok;
        a.x = nullptr, refused(e.call(a), "NULL operand", "x = NULL");
        a = e.ok, a.io = nullptr, refused(e.call(a), "NULL operand", "out / d_out = NULL");
        a = e.ok, a.C = 32, refused(e.call(a), "feature channels", "C = 32");
        a = e.ok, a.B = 0, refused(e.call(a), "at least 1", "B = 0");
        a = e.ok, a.D = 0, refused(e.call(a), "at least 1", "D = 0");
        a = e.ok, a.Hf = 300, refused(e.call(a), "Hf <= H", "Hf > H");
        a = e.ok, a.H = 1, a.Hf = 1, refused(e.call(a), "H, W >= 2", "H = 1");
        a = e.ok, a.H = a.W = a.Hf = a.Wf = 65536, refused(e.call(a), "too large", "Hf*Wf beyond int");
        a = e.ok, a.B = 65536, refused(e.call(a), "65535", "B beyond the grid");
        a = e.ok, a.B = 300, a.A = 300, refused(e.call(a), "65535", "B*A beyond the grid");
        a = e.ok, a.stride = 96 * 64 * 114 - 1, refused(e.call(a), "batch_stride", "a short batch stride");
        a = e.ok, a.fov = 0.f, refused(e.call(a), "fov_scale", "fov_scale = 0");
        workspace_refusals(e.who, e.ok.ws_bytes, [&](void* w, size_t n) { a = e.ok, a.ws = w, a.ws_bytes = n; return e.call(a); });
    }
    CvArgs a = ok_b;
    a.d_x = nullptr, a.d_xa = nullptr, refused(cv_bwd(a), "nothing to do", "both outputs NULL");
    a = ok_b, a.B = 64, a.A = 8, a.H = a.W = a.Hf = a.Wf = 512, a.stride = (int64_t)96 * 512 * 512;
    refused(cv_bwd(a), "corner contributions", "more contributions than the lists index");
    a = ok_b, a.d_x = nullptr, a.ws_bytes = 0, refused(cv_bwd(a), "workspace", "d_x = NULL alone is no refusal; the empty workspace is");
}

// ---- the reconstruction loss, both ways ----
struct RlArgs {
    const float *images, *alpha, *cams, *depth;
    const unsigned char* mask;
    float *out, *out2;                               // loss, - | d_depth, d_loss
    int64_t S, B;
    int A, H, W;
    float fov, zfar, f;
    int pad;
    void* ws;
    size_t ws_bytes;
};

static int rl_fwd(const RlArgs& a) {
    return mcr_reconstruction_loss(a.images, a.alpha, a.mask, a.cams, a.depth, a.out, nullptr, nullptr, a.S, a.B, a.A, a.H, a.W, a.fov, a.zfar, a.f,
                                   a.pad, a.ws, a.ws_bytes, nullptr);
}
static int rl_bwd(const RlArgs& a) {
    return mcr_reconstruction_loss_backward(a.images, a.alpha, a.mask, a.cams, a.depth, a.out2, a.out, a.S, a.B, a.A, a.H, a.W, a.fov, a.zfar, a.f,
                                            a.pad, a.ws, a.ws_bytes, nullptr);
}

static void reconstruction_loss_checks() {
    size_t (*sizes[])(int64_t, int64_t, int64_t, int64_t, int64_t) = {mcr_reconstruction_loss_workspace_bytes,
                                                                      mcr_reconstruction_loss_backward_workspace_bytes};
    for (auto size : sizes) {
        expect(size(0, 1, 2, 256, 456) == 0, "rl size, S = 0");
        expect(size(4, 1, 9, 256, 456) == 0, "rl size, A = 9");
        expect(size(4, 1, 2, 1, 456) == 0, "rl size, H = 1");
        expect(size(4, 65536, 2, 256, 456) == 0, "rl size, B beyond the grid");
        expect(size(4, 1, 2, INT64_MAX, 456) == 0, "rl size, H = INT64_MAX");
        expect(size(4, 1, 2, 1 << 16, 1 << 16) == 0, "rl size, H*W beyond int");
        expect(size(65535, 65535, 8, 1 << 15, 1 << 15) == 0, "rl size, everything large");
    }
    size_t prev = 0;
    for (int64_t H = 2; H <= 200; H += 17) {
        const size_t s = mcr_reconstruction_loss_workspace_bytes(4, 2, 2, H, 456);
        expect(s >= prev && s % 256 == 0 && s >= (size_t)4 * 2 * ((H + 15) / 16) * 29 * 8 + 4 * 2 * 8, "rl size: a float and an int per tile, a double per map");
        prev = s;
    }
    expect(mcr_reconstruction_loss_backward_workspace_bytes(4, 3, 2, 256, 456) >= 3 * 64 * sizeof(int), "rl bwd size: 64 counts an image");

    const RlArgs ok_f = {dummy, dummy, dummy, dummy, dummy_mask, dummy, dummy, 4, 1, 2, 256, 456, 1.7320508f, 10.f, 0.85f, 0, ws,
                         mcr_reconstruction_loss_workspace_bytes(4, 1, 2, 256, 456)};
    RlArgs ok_b = ok_f;
    ok_b.ws_bytes = mcr_reconstruction_loss_backward_workspace_bytes(4, 1, 2, 256, 456);
    struct { const char* who; const RlArgs& ok; int (*call)(const RlArgs&); } both[] = {{"rl", ok_f, rl_fwd}, {"rl bwd", ok_b, rl_bwd}};
    for (const auto& e : both) {
        RlArgs a = e.ok;
        a.images = nullptr, refused(e.call(a), "NULL operand", "images = NULL");
        a = e.ok, a.depth = nullptr, refused(e.call(a), "NULL operand", "depth = NULL");
        a = e.ok, a.out = nullptr, refused(e.call(a), "NULL", "loss / d_depth = NULL");
        a = e.ok, a.A = 9, refused(e.call(a), "sources", "A = 9");
        a = e.ok, a.W = 1, refused(e.call(a), "at least 2", "W = 1");
        a = e.ok, a.S = 0, refused(e.call(a), "at least 1", "S = 0");
        a = e.ok, a.pad = 2, refused(e.call(a), "padding mode", "padding mode 2");
        a = e.ok, a.H = a.W = 1 << 16, refused(e.call(a), "overflows an index", "H*W beyond int");
        a = e.ok, a.B = 65536, refused(e.call(a), "overflows an index", "B beyond the grid");
        a = e.ok, a.fov = -1.f, refused(e.call(a), "fov_scale", "fov_scale < 0");
        a = e.ok, a.zfar = INFINITY, refused(e.call(a), "zfar", "zfar = inf");
        a = e.ok, a.f = 1.5f, refused(e.call(a), "ssim_factor", "ssim_factor = 1.5");
        workspace_refusals(e.who, e.ok.ws_bytes, [&](void* w, size_t n) { a = e.ok, a.ws = w, a.ws_bytes = n; return e.call(a); });
    }
    RlArgs a = ok_b;
    a.out2 = nullptr, refused(rl_bwd(a), "NULL d_loss", "d_loss = NULL");
}

// ---- the disparity scales, both ways ----
struct DsArgs {
    const float* disps[8];
    float* d_disps[8];
    int Hs[8], Ws[8];
    const float* images;
    const float *d_depth, *d_reg;
    float* out;                                      // depth, reg and error_mask of the forward
    int S;
    int64_t B;
    int H, W;
    float znear, zfar;
    void* ws;
    size_t ws_bytes;
};

static int ds_fwd(const DsArgs& a) {
    return mcr_disparity_scales(a.disps, a.Hs, a.Ws, a.images, dummy_mask, a.out, a.out, (unsigned char*)a.out, nullptr, nullptr, a.S, a.B, a.H, a.W,
                                a.znear, a.zfar, a.ws, a.ws_bytes, nullptr);
}
static int ds_bwd(const DsArgs& a) {
    return mcr_disparity_scales_backward(a.disps, a.Hs, a.Ws, a.images, dummy_mask, a.d_depth, a.d_reg, a.d_disps, a.S, a.B, a.H, a.W, a.znear, a.zfar,
                                         a.ws, a.ws_bytes, nullptr);
}

static void disparity_scales_checks() {
    size_t (*sizes[])(int64_t, int64_t, int64_t, int64_t) = {mcr_disparity_scales_workspace_bytes, mcr_disparity_scales_backward_workspace_bytes};
    for (auto size : sizes) {
        expect(size(0, 1, 256, 456) == 0, "ds size, S = 0");
        expect(size(9, 1, 256, 456) == 0, "ds size, S = 9");
        expect(size(4, 65536, 256, 456) == 0, "ds size, B beyond the grid");
        expect(size(4, 1, 256, 1) == 0, "ds size, W = 1");
        expect(size(4, 1, INT64_MAX, 456) == 0, "ds size, H = INT64_MAX");
        expect(size(4, 1, 1 << 16, 1 << 16) == 0, "ds size, H*W beyond int");
        expect(size(8, 65535, 1 << 15, 1 << 15) == 0, "ds size, everything large");
        size_t prev = 0;
        for (int64_t B = 1; B <= 40; B += 3) {
            const size_t s = size(4, B, 250, 456);
            expect(s > prev && s % 256 == 0 && s >= (size_t)4 * B * 32 * 8, "ds size grows with B and holds the chunk sums");
            prev = s;
        }
    }
    expect(mcr_disparity_scales_workspace_bytes(4, 2, 256, 456) >= (size_t)2 * 256 * 456 * 4, "ds size holds the table");

    DsArgs ok_f = {};
    for (int s = 0; s < 4; ++s) ok_f.disps[s] = dummy, ok_f.d_disps[s] = dummy, ok_f.Hs[s] = 256 >> s, ok_f.Ws[s] = 456 >> s;
    ok_f.images = dummy, ok_f.d_depth = dummy, ok_f.d_reg = dummy, ok_f.out = dummy;
    ok_f.S = 4, ok_f.B = 2, ok_f.H = 256, ok_f.W = 456, ok_f.znear = 0.5f, ok_f.zfar = 10.f, ok_f.ws = ws;
    DsArgs ok_b = ok_f;
    ok_f.ws_bytes = mcr_disparity_scales_workspace_bytes(4, 2, 256, 456), ok_b.ws_bytes = mcr_disparity_scales_backward_workspace_bytes(4, 2, 256, 456);
    struct { const char* who; const DsArgs& ok; int (*call)(const DsArgs&); } both[] = {{"ds", ok_f, ds_fwd}, {"ds bwd", ok_b, ds_bwd}};
    for (const auto& e : both) {
        DsArgs a = e.ok;
        a.S = 9, refused(e.call(a), "scales", "S = 9");
        a = e.ok, a.images = nullptr, refused(e.call(a), "NULL operand", "images = NULL");
        a = e.ok, a.disps[2] = nullptr, refused(e.call(a), "NULL map of scale 2", "disps[2] = NULL");
        a = e.ok, a.H = 1, refused(e.call(a), "at least 2", "H = 1");
        a = e.ok, a.B = 0, refused(e.call(a), "at least 1", "B = 0");
        a = e.ok, a.B = 65536, refused(e.call(a), "overflows an index", "B beyond the grid");
        a = e.ok, a.znear = 0.f, refused(e.call(a), "znear and zfar", "znear = 0");
        a = e.ok, a.Hs[1] = 0, refused(e.call(a), "scale 1 is", "an empty scale");
        a = e.ok, a.Hs[1] = 100, refused(e.call(a), "the ratio must be", "a ratio that is no power of two");
        a = e.ok, a.Ws[3] = 100, refused(e.call(a), "one ratio on both axes", "two ratios");
        workspace_refusals(e.who, e.ok.ws_bytes, [&](void* w, size_t n) { a = e.ok, a.ws = w, a.ws_bytes = n; return e.call(a); });
    }
    DsArgs a = ok_f;
    a.out = nullptr, refused(ds_fwd(a), "NULL depth", "depth = NULL");
    a = ok_b, a.d_disps[1] = nullptr, refused(ds_bwd(a), "NULL map of scale 1", "d_disps[1] = NULL");
    a = ok_b, a.d_depth = nullptr, a.d_reg = nullptr, refused(ds_bwd(a), "nothing to do", "both gradients NULL");
}

int main() {
    ws = aligned_alloc(256, 4096);
    cost_volume_checks();
    reconstruction_loss_checks();
    disparity_scales_checks();
    free(ws);
    printf(failures ? "%d checks failed\n" : "all host checks passed\n", failures);
    return failures != 0;
}
