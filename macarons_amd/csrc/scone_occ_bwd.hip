// SconeOcc backward (SconeOcc.py:250-347): mcr_scone_occ_backward, the network around the four PCTransformers behind one entry, given
// the neighbour indices.  The global transformer's forward runs once; then, cloud by cloud and chunk by chunk of its queries, the
// neighbourhoods are gathered as offsets (so_gather_kernel), the three local transformers, the x-embedding and the head run forward and
// backward on the chunk functions of pct_bwd.hip (pb_chunk_forward / pb_chunk_backward) and the launchers of bwd_kernels.h; the query's share of the
// offsets' gradient is so_dx_sub_kernel.  Weight gradients of the chunks behind the first are staged and added in chunk order, as are
// the chunks' column sums of the global features' gradient; the global transformer's backward runs last.  No gradient for the clouds.
//
// Ragged SconeOcc backward: mcr_scone_occ_backward_ragged, the gradient of J such calls of different sizes (the jobs of
// SconeOcc.forward_ragged) with the weight gradients summed over the jobs.  The neighbourhood offsets are an input, so everything but
// the global features is row-wise: the rows of all jobs are packed into full chunks that run the same chunk function
// (so_chunk_fwd_bwd).  The global transformer runs forward over the J padded sequences with their lengths (keys masked, pooling over
// the valid rows; so_pad_global_kernel first overwrites the padding), its features reach the rows through so_bcast_rows_kernel, their
// gradient comes back per job through so_seg_colsum_kernel, and its backward runs last, job by job in job order with lengths
// (pb_pool_bwd_lens_kernel hands exact zeros to the padded rows), the jobs behind the first through a staging area.
// (Numerics and determinism: as stated in scone_vis_bwd.hip, for every entry of the backward sources.)
#include "bwd_kernels.h"

namespace mcr {
namespace {
// ---- SconeOcc (SconeOcc.py:250-347): the network around the four PCTransformers -------------------------------------------------------
constexpr int SO_K = 16;                                            // neighbours per query and scale
constexpr int SO_G = 512, SO_LF = 256, SO_XE = 512, SO_VH = 64;     // widths of the head's input: global | 3 x local | x-embedding | harmonics
constexpr int SO_LOC = SO_G, SO_XCOL = SO_LOC + 3 * SO_LF, SO_VCOL = SO_XCOL + SO_XE, SO_H = SO_VCOL + SO_VH;   // its columns (1856 in all)
constexpr int SO_L1 = 512, SO_L2 = 256;                             // the head's hidden widths
constexpr int SO_HEAD_NW = 6 * LIN_NW;                              // x_embedding.linear{1,2,3}, linear{1,2,3}: the table from OCC_XE on
static_assert(SO_H == 1856 && OCC_LIN == OCC_XE + 3 * LIN_NW && SO_HEAD_NW <= PCT_NW, "SconeOcc head layout");

// its six layers, in table order: the x-embedding's three, the head's three
constexpr LinShape SO_XE1{SO_XE / 4, 3}, SO_XE2{SO_XE / 2, SO_XE / 4}, SO_XE3{SO_XE, SO_XE / 2}, SO_LIN1{SO_L1, SO_H}, SO_LIN2{SO_L2, SO_L1},
    SO_LIN3{1, SO_L2};
constexpr LinShape SO_HEAD[SO_HEAD_NW / LIN_NW] = {SO_XE1, SO_XE2, SO_XE3, SO_LIN1, SO_LIN2, SO_LIN3};

// floats of the table entry OCC_XE + slot
inline int so_head_slot_floats(int slot) { return lin_slot_floats(SO_HEAD[slot / LIN_NW], slot % LIN_NW); }

// off[(r*16 + j)*3 + c] = pc[idx[r*16 + j]*3 + c] - x[r*3 + c]: the neighbourhoods of `rows` queries of one cloud of M points, as offsets
// (SconeOcc.py:296-300; the fp32 subtraction torch performs).  One thread per (query, neighbour); an index outside the cloud is clamped
// into it (never an access out of bounds).
__global__ __launch_bounds__(256) void so_gather_kernel(const float* __restrict__ pc, long long M, const long long* __restrict__ idx,
                                                        const float* __restrict__ x, float* __restrict__ off, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * SO_K) return;
    const long long r = e / SO_K;
    const long long i = min(max(idx[e], 0ll), M - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) off[e * 3 + c] = pc[i * 3 + c] - x[r * 3 + c];
}

// d_x[r*3 + c] -= sum_j d_off[(r*16 + j)*3 + c], j ascending: the query's share of its neighbourhood's offsets.  One thread per (query,
// channel) owns its output: no atomics.
__global__ __launch_bounds__(256) void so_dx_sub_kernel(const float* __restrict__ d_off, float* __restrict__ d_x, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * 3) return;
    const long long r = e / 3;
    const int c = (int)(e - r * 3);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < SO_K; ++j) acc += d_off[(r * SO_K + j) * 3 + c];
    d_x[e] -= acc;
}

void launch_so_gather(hipStream_t s, const float* pc, int64_t M, const int64_t* idx, const float* x, float* off, int64_t rows) {
    hipLaunchKernelGGL(so_gather_kernel, dim3((unsigned)cdiv(rows * SO_K, 256)), dim3(256), 0, s, pc, (long long)M, (const long long*)idx, x, off,
                       (long long)rows);
}
void launch_so_dx_sub(hipStream_t s, const float* d_off, float* d_x, int64_t rows) {
    hipLaunchKernelGGL(so_dx_sub_kernel, dim3((unsigned)cdiv(rows * 3, 256)), dim3(256), 0, s, d_off, d_x, (long long)rows);
}

inline int64_t so_chunk(int64_t Q, int64_t q_chunk) { return std::min<int64_t>(q_chunk > 0 ? q_chunk : PB_CHUNK16, Q); }

// The workspace of mcr_scone_occ_backward: what outlives a chunk (the global features and their gradient), then one chunk of Qc queries
// OVER the global transformer's scratch -- the two are never alive together (the global forward runs first, its backward last).
struct SoScratch {
    float *gfeat, *dG, *gtmp;                              // [B, 512] global features and their gradient; one chunk's partial of a row of it
    float *off[3], *d_off;                                 // the chunk's neighbourhoods [Qc, 16, 3] per scale; the gradient of one of them
    float *ze1, *ge1, *ze2, *ge2, *ze3;                    // x-embedding: pre-activations and GELUs
    float *h, *z1, *g1, *z2, *g2, *z3;                     // head: input [Qc, 1856], pre-activations and GELUs
    float *dH, *d1, *d2, *dz3;                             // gradients: head input; 512- and 256-wide layers (the x-embedding's 128 / 256 too); output
    float *part, *wt;                                      // weight-gradient slabs; transposed weight
    float* stage;                                          // weight gradients of the chunks behind the first: 3 PCT tables, then the head's
    PbScratch local[3];                                    // one 16-token chunk per scale: each keeps what its forward leaves (boundaries, embedding
                                                           // and tail), the three share the encoder interior and the gradient buffers
    PbScratch global;                                      // B sequences of Lg tokens
};
// one chunk of Qc queries (everything of SoScratch but what outlives a chunk and the global transformer's scratch)
void carve_so_chunk(Arena& c, SoScratch& w, int64_t Qc) {
    for (float*& o : w.off) o = c.f(Qc * SO_K * 3);
    w.d_off = c.f(Qc * SO_K * 3);
    w.ze1 = c.f(Qc * (SO_XE / 4)); w.ge1 = c.f(Qc * (SO_XE / 4)); w.ze2 = c.f(Qc * (SO_XE / 2)); w.ge2 = c.f(Qc * (SO_XE / 2));
    w.ze3 = c.f(Qc * SO_XE);
    w.h = c.f(Qc * SO_H); w.z1 = c.f(Qc * SO_L1); w.g1 = c.f(Qc * SO_L1); w.z2 = c.f(Qc * SO_L2); w.g2 = c.f(Qc * SO_L2); w.z3 = c.f(Qc);
    w.dH = c.f(Qc * SO_H); w.d1 = c.f(Qc * SO_L1); w.d2 = c.f(Qc * SO_L2); w.dz3 = c.f(Qc);
    size_t n_part = 0, n_stage = 3 * pb_stage_floats(SO_LF / 2);
    for (const LinShape& l : SO_HEAD) n_part = std::max(n_part, vb_gradw_floats(Qc, l.N, l.K));
    for (int i = 0; i < SO_HEAD_NW; ++i) n_stage += so_head_slot_floats(i);
    w.part = c.f(n_part);
    w.wt = c.f((size_t)SO_LIN1.N * SO_LIN1.K);
    w.stage = c.f(n_stage);
    w.local[0] = carve_pb_chunk(c, Qc, SO_K, SO_LF / 2, false);
    for (int i = 1; i < 3; ++i) {
        PbScratch& l = w.local[i];
        const int64_t T = Qc * SO_K;
        l = w.local[0];
        for (float*& x : l.X) x = c.f(T * PB_E);
        l.z1 = c.f(T * PB_F); l.g1 = c.f(T * PB_F);
        l.hn = c.f(T * PB_E); l.y0 = c.f(T * (SO_LF / 2));
    }
}
SoScratch carve_so(Arena& a, int64_t B, int64_t Qc, int64_t Lg) {
    SoScratch w;
    w.gfeat = a.f(B * SO_G); w.dG = a.f(B * SO_G); w.gtmp = a.f(SO_G);
    Arena c = a.rest(), g = a.rest();
    carve_so_chunk(c, w, Qc);
    w.global = carve_pb_chunk(g, B, Lg, SO_G / 2, false);
    a.off += std::max(c.off, g.off);
    return w;
}

// The workspace of mcr_scone_occ_backward_ragged: as SoScratch over J jobs (so.global: the J padded sequences' forward), plus the padded
// sequences with their padding overwritten, and ONE sequence's scratch for the global transformer's backward, which runs job by job
// (the jobs behind the first through a staging area of their own)
struct SoRaggedScratch {
    SoScratch so;
    float* pcg;                                            // [J, Lg, 3]: pc_global, rows >= the length = the sequence's row 0
    PbScratch global1;                                     // one sequence of Lg tokens (with its staging area)
};
SoRaggedScratch carve_so_ragged(Arena& a, int64_t J, int64_t Qc, int64_t Lg) {
    SoRaggedScratch r;
    SoScratch& w = r.so;
    w.gfeat = a.f(J * SO_G); w.dG = a.f(J * SO_G); w.gtmp = nullptr;
    r.pcg = a.f(J * Lg * 3);
    Arena c = a.rest(), g = a.rest(), g1 = a.rest();
    carve_so_chunk(c, w, Qc);
    w.global = carve_pb_chunk(g, J, Lg, SO_G / 2, false);
    r.global1 = carve_pb_chunk(g1, 1, Lg, SO_G / 2, true);
    a.off += std::max({c.off, g.off, g1.off});
    return r;
}

// ---- the ragged pass: rows of J jobs packed into chunks -------------------------------------------------------------------------------
// dst[(j*L + r)*3 + c] = src[(j*L + (r < n ? r : 0))*3 + c], n = min(L, max(1, lens[j])): the padded sequences with their padding
// overwritten by a valid row.  The forward masks the padded keys, but the weight-gradient products of the backward multiply every row's
// (zero) gradient with what the row holds: 0 x NaN would be NaN.  One thread per (row, channel).
__global__ __launch_bounds__(256) void so_pad_global_kernel(const float* __restrict__ src, const int* __restrict__ lens,
                                                            float* __restrict__ dst, long long J, int L) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= J * L * 3) return;
    const long long row = e / 3;
    const int c = (int)(e - row * 3);
    const long long j = row / L;
    const int r = (int)(row - j * L);
    const int n = min(L, max(1, lens[j]));
    dst[e] = src[(j * L + (r < n ? r : 0)) * 3 + c];
}

// h[r*ldh + c] = gfeat[row_job[r]*512 + c] (c < 512): every row's job's global features into the head's input.  One thread per (row,
// column), consecutive threads on consecutive columns; a job outside [0, J) is clamped into it (never an access out of bounds).
__global__ __launch_bounds__(256) void so_bcast_rows_kernel(const float* __restrict__ gfeat, const int* __restrict__ row_job, long long J,
                                                            float* __restrict__ h, long long ldh, long long rows) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= rows * SO_G) return;
    const long long r = e / SO_G;
    const int c = (int)(e - r * SO_G);
    const long long j = min(max((long long)row_job[r], 0ll), J - 1);
    h[r * ldh + c] = gfeat[j * SO_G + c];
}

// dG[j*512 + c] += sum of dH[(r - r0)*ldh + c] over the rows r of job j inside the chunk [r0, r0 + rows), r ascending; job j = rows
// [job_rows[j], job_rows[j + 1]) (clamped into the chunk: never an access out of bounds).  One thread owns each (j, c): no atomics, and
// the chunks run one behind the other on the stream, so the sum has one order.  A job without rows in the chunk is left alone.
__global__ __launch_bounds__(256) void so_seg_colsum_kernel(const float* __restrict__ dH, long long ldh, const long long* __restrict__ job_rows,
                                                            long long J, long long r0, long long rows, float* __restrict__ dG) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= J * SO_G) return;
    const long long j = e / SO_G;
    const int c = (int)(e - j * SO_G);
    const long long lo = min(max(job_rows[j], r0), r0 + rows) - r0, hi = min(max(job_rows[j + 1], r0), r0 + rows) - r0;
    if (lo >= hi) return;
    float acc = 0.f;
#pragma unroll 8
    for (long long r = lo; r < hi; ++r) acc += dH[r * ldh + c];
    dG[e] += acc;
}

// How a chunk's rows meet the global features: all of one cloud (row_job NULL: gfeat / dG are that cloud's rows of 512, and the cloud's
// first chunk writes dG where the later ones add), or every row with its job (gfeat / dG [J, 512]; row_job: the chunk's slice, r0: its
// first row)
struct SoGlobalRows {
    const float* gfeat; float* dG; float* gtmp; bool first_of_cloud;
    const int* row_job; const long long* job_rows; int64_t J, r0;
};


// the chunks behind the first leave their weight gradients in the staging area, cut in table order, and are added in chunk order:
// the three local transformers' tables, then the head's; tab: the table such a chunk is handed (d_weights NULL: nothing is staged)
struct SoStages {
    float* tab[OCC_NW] = {};
    Stage part[4];
    SoStages(float* const* d_weights, float* stage) {
        if (!d_weights) return;
        for (int i = 0; i < 3; ++i) {
            const int o = OCC_LOCAL + i * PCT_NW;
            part[i] = Stage(d_weights + o, tab + o, stage, PCT_NW, [](int k) { return pb_slot_floats(k, SO_LF / 2); });
            stage += part[i].floats();
        }
        part[3] = Stage(d_weights + OCC_XE, tab + OCC_XE, stage, SO_HEAD_NW, so_head_slot_floats);
    }
    void add(hipStream_t s) const { for (const Stage& p : part) p.add(s); }
};

// One chunk of n rows, forward and backward, given its neighbourhoods as offsets off[i] [n, 16, 3]: (b) the local features, (c) the
// x-embedding, (d) the head, then (e) - (h) their backward.  xc / vhc / d_out_c / dxc / dvhc: the chunk's rows of the operands (dxc, dvhc
// may be NULL); dw: where this chunk's weight gradients go (NULL: none wanted); deep: anything below the head's input wanted
void so_chunk_fwd_bwd(hipStream_t s, const OccW& w, const SoScratch& ws, const float* const* off, const float* xc, const float* vhc,
                      const float* d_out_c, int64_t n, float* const* dw, float* dxc, float* dvhc, bool deep, const SoGlobalRows& g) {
    const LinCtx c{s, n, ws.part, ws.wt, dw};
    constexpr int XE1 = OCC_XE, XE2 = OCC_XE + LIN_NW, XE3 = OCC_XE + 2 * LIN_NW, LIN1 = OCC_LIN, LIN2 = OCC_LIN + LIN_NW, LIN3 = OCC_LIN + 2 * LIN_NW;
    // (b) the local features, straight into the head's input
    for (int i = 0; i < 3; ++i) {
        pb_chunk_forward(s, w.local[i], off[i], n, SO_K, SO_LF / 2, ws.local[i]);
        launch_pool_max_avg(s, ws.local[i].y0, SO_LF / 2, ws.h + SO_LOC + i * SO_LF, SO_H, n, SO_K, SO_LF / 2);
    }
    // (c) the x-embedding (SconeOcc.py:7-42)
    lin_fwd(s, n, SO_XE1, w.xe1, {xc, 3}, {}, {ws.ze1, SO_XE / 4}, {ws.ge1, SO_XE / 4});
    lin_fwd(s, n, SO_XE2, w.xe2, {ws.ge1, SO_XE / 4}, {}, {ws.ze2, SO_XE / 2}, {ws.ge2, SO_XE / 2});
    lin_fwd(s, n, SO_XE3, w.xe3, {ws.ge2, SO_XE / 2}, {}, {ws.ze3, SO_XE}, {ws.h + SO_XCOL, SO_H});
    // (d) the head (SconeOcc.py:334-342): GELU behind every layer, the last included
    if (g.row_job)
        hipLaunchKernelGGL(so_bcast_rows_kernel, dim3((unsigned)cdiv(n * SO_G, 256)), dim3(256), 0, s, g.gfeat, g.row_job, (long long)g.J, ws.h,
                           (long long)SO_H, (long long)n);
    else launch_copy2d(s, g.gfeat, 0, ws.h, SO_H, n, SO_G);
    launch_copy2d(s, vhc, SO_VH, ws.h + SO_VCOL, SO_H, n, SO_VH);
    lin_fwd(s, n, SO_LIN1, w.lin1, {ws.h, SO_H}, {}, {ws.z1, SO_L1}, {ws.g1, SO_L1});
    lin_fwd(s, n, SO_LIN2, w.lin2, {ws.g1, SO_L1}, {}, {ws.z2, SO_L2}, {ws.g2, SO_L2});
    lin_fwd(s, n, SO_LIN3, w.lin3, {ws.g2, SO_L2}, {}, {ws.z3, 1});
    // (e) the head, backwards
    launch_copy2d(s, d_out_c, 1, ws.dz3, 1, n, 1);
    lin_bwd(c, SO_LIN3, w.lin3, LIN3, {ws.z3, 1}, {ws.dz3, 1}, {ws.g2, SO_L2}, {ws.d2, SO_L2});
    lin_bwd(c, SO_LIN2, w.lin2, LIN2, {ws.z2, SO_L2}, {ws.d2, SO_L2}, {ws.g1, SO_L1}, {ws.d1, SO_L1});
    lin_bwd(c, SO_LIN1, w.lin1, LIN1, {ws.z1, SO_L1}, {ws.d1, SO_L1}, {ws.h, SO_H}, {ws.dH, SO_H});
    // (f) what leaves the head's input as it is: the harmonics' columns, the global features' (summed over the chunk's rows -- one
    // cloud: the bias half of a weight-gradient product of depth 0, then chunk by chunk in order; jobs: so_seg_colsum_kernel)
    if (dvhc) launch_copy2d(s, ws.dH + SO_VCOL, SO_H, dvhc, SO_VH, n, SO_VH);
    if (!deep) return;
    if (dw && g.row_job) {
        hipLaunchKernelGGL(so_seg_colsum_kernel, dim3((unsigned)cdiv(g.J * SO_G, 256)), dim3(256), 0, s, (const float*)ws.dH, (long long)SO_H,
                           g.job_rows, (long long)g.J, (long long)g.r0, (long long)n, g.dG);
    } else if (dw) {
        float* const colsum[LIN_NW] = {nullptr, g.first_of_cloud ? g.dG : g.gtmp};      // (as a layer's [dW | db]: no dW, db = the sums)
        lin_bwd({s, n, ws.part, ws.wt, colsum}, LinShape{SO_G, 0}, {}, 0, {}, {ws.dH, SO_H}, {});
        if (!g.first_of_cloud) Stage(&g.dG, nullptr, g.gtmp, 1, [](int) { return SO_G; }).add(s, 2);   // one row of the global features' gradient
    }
    // (g) the x-embedding, backwards
    float* dxe = ws.dH + SO_XCOL;
    lin_bwd(c, SO_XE3, w.xe3, XE3, {ws.ze3, SO_XE}, {dxe, SO_H}, {ws.ge2, SO_XE / 2}, {ws.d2, SO_XE / 2});
    lin_bwd(c, SO_XE2, w.xe2, XE2, {ws.ze2, SO_XE / 2}, {ws.d2, SO_XE / 2}, {ws.ge1, SO_XE / 4}, {ws.d1, SO_XE / 4});
    lin_bwd(c, SO_XE1, w.xe1, XE1, {ws.ze1, SO_XE / 4}, {ws.d1, SO_XE / 4}, {xc, 3}, {dxc, 3});
    // (h) the local transformers, backwards, from what (b) left in each scale's scratch (no second forward; each encoder's
    // interior is rebuilt from its boundary as ever); the query's share of the offsets
    for (int i = 0; i < 3; ++i) {
        pb_chunk_backward(s, w.local[i], off[i], ws.dH + SO_LOC + i * SO_LF, n, SO_K, SO_LF / 2, dw ? dw + OCC_LOCAL + i * PCT_NW : nullptr,
                          dxc ? ws.d_off : nullptr, ws.local[i], SO_H, /*forward_done=*/true);
        if (dxc) launch_so_dx_sub(s, ws.d_off, dxc, n);
    }
}

constexpr int64_t SO_RAGGED_MAX_J = 16384;                           // jobs of one mcr_scone_occ_backward_ragged call

// What the two entries check alike, in two parts (the ragged entry has a check of its own between them): the chunk size and the
// operands' alignment; the workspace and the gradient table
int so_check_operands(const char* who, int64_t q_chunk, const float* pc_global, const float* x, const float* view_harmonics, const float* d_out,
                      const float* d_x, const float* d_view_harmonics) {
    MCR_REQUIRE(q_chunk == 0 || (q_chunk >= 16 && q_chunk % 16 == 0 && q_chunk <= (1 << 20)),
                "%s: q_chunk must be 0 (the default) or a multiple of 16 in [16, 2^20], got %ld", who, (long)q_chunk);
    MCR_REQUIRE(((uintptr_t)pc_global | (uintptr_t)x | (uintptr_t)view_harmonics | (uintptr_t)d_out | (uintptr_t)d_x |
                 (uintptr_t)d_view_harmonics) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    return 0;
}
int so_check_buffers(const char* who, const void* workspace, size_t workspace_bytes, size_t need, float* const* d_weights) {
    if (check_bwd_workspace(who, workspace, workspace_bytes, need)) return 1;
    return check_d_weights(who, d_weights, OCC_NW);
}
}  // namespace
}  // namespace mcr
using namespace mcr;
extern "C" {
// ---- SconeOcc ------------------------------------------------------------------------------------------------------------------------
int mcr_scone_occ_backward_chunk(int64_t Q) { return Q > 0 ? (int)so_chunk(Q, 0) : 0; }

size_t mcr_scone_occ_backward_workspace_bytes(int64_t B, int64_t Q, int64_t Lg, int64_t q_chunk) {
    return (B > 0 && Q > 0 && Lg > 0 && q_chunk >= 0) ? measure(carve_so, B, so_chunk(Q, q_chunk), Lg) + VB_WS_SLACK : 0;
}

int mcr_scone_occ_backward(const float* pc_global, int64_t Lg, const float* const* pc_scale, const int64_t* M_scale, const float* x,
                           const float* view_harmonics, const int64_t* const* knn_idx, const float* d_out, int64_t B, int64_t Q,
                           const float* const* weights, int n_weights, float* const* d_weights, float* d_x, float* d_view_harmonics,
                           int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_occ_backward";
    MCR_REQUIRE(pc_global && pc_scale && M_scale && x && view_harmonics && knn_idx && d_out && weights, "%s: null pointer", who);
    if (check_table(who, OCC_TABLE, weights, n_weights, OCC_NW)) return 1;                  // (the planes tails are accepted and ignored)
    MCR_REQUIRE(B > 0 && Q > 0 && Lg > 0 && B <= 65535 && Q <= (1ll << 24) && Lg <= (1 << 24) && B <= (1ll << 31) / Lg &&
                    (Lg != SO_K || B <= PB_CHUNK16),
                "%s: bad problem size B=%ld Q=%ld Lg=%ld", who, (long)B, (long)Q, (long)Lg);
    for (int i = 0; i < 3; ++i) {
        MCR_REQUIRE(pc_scale[i] && knn_idx[i], "%s: scale %d: null pointer", who, i);
        MCR_REQUIRE(M_scale[i] >= SO_K, "%s: scale %d has %ld points (< k = 16)", who, i, (long)M_scale[i]);
        MCR_REQUIRE(((uintptr_t)pc_scale[i] | (uintptr_t)knn_idx[i]) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    }
    if (so_check_operands(who, q_chunk, pc_global, x, view_harmonics, d_out, d_x, d_view_harmonics)) return 1;
    if (so_check_buffers(who, workspace, workspace_bytes, mcr_scone_occ_backward_workspace_bytes(B, Q, Lg, q_chunk), d_weights)) return 1;
    if (!d_weights && !d_x && !d_view_harmonics) return 0;
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, OCC_NW);
    const int64_t Qc = so_chunk(Q, q_chunk);
    Arena a{(char*)workspace, workspace_bytes};
    const SoScratch ws = carve_so(a, B, Qc, Lg);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const bool deep = d_weights || d_x;                    // anything below the head's input wanted
    const SoStages st(d_weights, ws.stage);

    // ---- 1. the global transformer's forward: [B, 512]
    pb_chunk_forward(s, w.global, pc_global, B, (int)Lg, SO_G / 2, ws.global);
    launch_pool_max_avg(s, ws.global.y0, SO_G / 2, ws.gfeat, SO_G, B, (int)Lg, SO_G / 2);

    // ---- 2. cloud by cloud, chunk by chunk
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q0 = 0; q0 < Q; q0 += Qc) {
            const int64_t n = std::min(Qc, Q - q0), r0 = b * Q + q0;
            const bool first = b == 0 && q0 == 0;
            // (a) the neighbourhoods as offsets
            for (int i = 0; i < 3; ++i)
                launch_so_gather(s, pc_scale[i] + b * M_scale[i] * 3, M_scale[i], knn_idx[i] + r0 * SO_K, x + r0 * 3, ws.off[i], n);
            so_chunk_fwd_bwd(s, w, ws, ws.off, x + r0 * 3, view_harmonics + r0 * SO_VH, d_out + r0, n,
                             !d_weights ? nullptr : first ? d_weights : st.tab, d_x ? d_x + r0 * 3 : nullptr,
                             d_view_harmonics ? d_view_harmonics + r0 * SO_VH : nullptr, deep,
                             SoGlobalRows{ws.gfeat + b * SO_G, ws.dG + b * SO_G, ws.gtmp, q0 == 0, nullptr, nullptr, 0, 0});
            if (deep && d_weights && !first) st.add(s);
        }

    // ---- 3. the global transformer, backwards (its forward is rebuilt: the chunks have used its scratch)
    if (d_weights) pb_chunk_backward(s, w.global, pc_global, ws.dG, B, (int)Lg, SO_G / 2, d_weights + OCC_GLOBAL, nullptr, ws.global, SO_G);
    MCR_LAUNCH_CHECK(who);
    return 0;
}

// ---- SconeOcc, ragged: J jobs of different sizes, their rows packed into chunks ----------------------------------------------------------
size_t mcr_scone_occ_backward_ragged_workspace_bytes(int64_t J, int64_t T, int64_t Lg, int64_t q_chunk) {
    return (J > 0 && T > 0 && Lg > 0 && q_chunk >= 0) ? measure(carve_so_ragged, J, so_chunk(T, q_chunk), Lg) + VB_WS_SLACK : 0;
}

int mcr_scone_occ_backward_ragged(const float* pc_global, const int* global_len, int64_t Lg, const float* const* offsets, const float* x,
                                  const float* view_harmonics, const int* row_job, const int64_t* job_rows, const float* d_out, int64_t J,
                                  int64_t T, const float* const* weights, int n_weights, float* const* d_weights, float* d_x,
                                  float* d_view_harmonics, int64_t q_chunk, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mcr_scone_occ_backward_ragged";
    MCR_REQUIRE(pc_global && global_len && offsets && x && view_harmonics && row_job && job_rows && d_out && weights, "%s: null pointer", who);
    if (check_table(who, OCC_TABLE, weights, n_weights, OCC_NW)) return 1;                  // (the planes tails are accepted and ignored)
    MCR_REQUIRE(J > 0 && T > 0 && Lg > 0 && J <= SO_RAGGED_MAX_J && T <= (1ll << 24) && Lg <= (1 << 24) && J <= (1ll << 31) / Lg,
                "%s: bad problem size J=%ld T=%ld Lg=%ld (J <= %ld)", who, (long)J, (long)T, (long)Lg, (long)SO_RAGGED_MAX_J);
    MCR_REQUIRE(Lg != SO_K, "%s: global sequences of 16 tokens are not supported (their fused attention backward takes no lens)", who);
    for (int i = 0; i < 3; ++i) {
        MCR_REQUIRE(offsets[i], "%s: scale %d: null pointer", who, i);
        MCR_REQUIRE((uintptr_t)offsets[i] % 16 == 0, "%s: operands must be 16-byte aligned", who);
    }
    if (so_check_operands(who, q_chunk, pc_global, x, view_harmonics, d_out, d_x, d_view_harmonics)) return 1;
    MCR_REQUIRE((uintptr_t)global_len % 4 == 0 && (uintptr_t)row_job % 4 == 0 && (uintptr_t)job_rows % 8 == 0,
                "%s: global_len, row_job (4 bytes) and job_rows (8 bytes) must be aligned to their element", who);
    if (so_check_buffers(who, workspace, workspace_bytes, mcr_scone_occ_backward_ragged_workspace_bytes(J, T, Lg, q_chunk), d_weights)) return 1;
    if (!d_weights && !d_x && !d_view_harmonics) return 0;
    hipStream_t s = (hipStream_t)stream;
    const OccW w = read_occ_table(weights, OCC_NW);
    const int64_t Qc = so_chunk(T, q_chunk);
    Arena a{(char*)workspace, workspace_bytes};
    const SoRaggedScratch rs = carve_so_ragged(a, J, Qc, Lg);
    MCR_REQUIRE(a.ok(), "%s: workspace overflow", who);
    const SoScratch& ws = rs.so;
    const bool deep = d_weights || d_x;
    const SoStages st(d_weights, ws.stage);

    // ---- 1. the global transformer's forward over the J padded sequences: [J, 512]; nothing of the caller's padding is read again
    hipLaunchKernelGGL(so_pad_global_kernel, dim3((unsigned)cdiv(J * Lg * 3, 256)), dim3(256), 0, s, pc_global, global_len, rs.pcg, (long long)J,
                       (int)Lg);
    pb_chunk_forward(s, w.global, rs.pcg, J, (int)Lg, SO_G / 2, ws.global, global_len);
    launch_pool_max_avg(s, ws.global.y0, SO_G / 2, ws.gfeat, SO_G, J, (int)Lg, SO_G / 2, global_len);
    if (d_weights)
        if (int e = check_hip(hipMemsetAsync(ws.dG, 0, (size_t)J * SO_G * sizeof(float), s), who)) return e;

    // ---- 2. the rows of all jobs, chunk by chunk
    const float* off[3];
    for (int64_t r0 = 0; r0 < T; r0 += Qc) {
        const int64_t n = std::min(Qc, T - r0);
        for (int i = 0; i < 3; ++i) off[i] = offsets[i] + r0 * SO_K * 3;
        so_chunk_fwd_bwd(s, w, ws, off, x + r0 * 3, view_harmonics + r0 * SO_VH, d_out + r0, n, !d_weights ? nullptr : r0 == 0 ? d_weights : st.tab,
                         d_x ? d_x + r0 * 3 : nullptr, d_view_harmonics ? d_view_harmonics + r0 * SO_VH : nullptr, deep,
                         SoGlobalRows{ws.gfeat, ws.dG, nullptr, false, row_job + r0, (const long long*)job_rows, J, r0});
        if (deep && d_weights && r0 > 0) st.add(s);
    }

    // ---- 3. the global transformer, backwards, job by job in job order (its forward is rebuilt: the chunks have used its scratch).  One
    // job's gradient depends on nothing but that job -- a job without rows has dG = 0 and adds exact zeros
    if (d_weights) {
        float* stage_tab[PCT_NW];
        const Stage stage(d_weights + OCC_GLOBAL, stage_tab, rs.global1.stage, PCT_NW, [](int k) { return pb_slot_floats(k, SO_G / 2); });
        for (int64_t j = 0; j < J; ++j) {
            pb_chunk_backward(s, w.global, rs.pcg + j * Lg * 3, ws.dG + j * SO_G, 1, (int)Lg, SO_G / 2, j == 0 ? d_weights + OCC_GLOBAL : stage_tab,
                              nullptr, rs.global1, SO_G, false, global_len + j);
            if (j > 0) stage.add(s);
        }
    }
    MCR_LAUNCH_CHECK(who);
    return 0;
}

}  // extern "C"
