"""Thin torch-tensor wrappers over the C ABI (include/macarons_hip.h).

torch is plumbing here: device memory, streams.  Every function validates layout, allocates outputs /
scratch on the input's device and launches on the current HIP stream.  No CPU fallback.
"""
import os
import ctypes
import torch
import numpy as np

from ._lib import lib, check, MacaronsHipError, c_i64, c_int, c_size, c_vp, c_f32
from .utility.host import limit_host_threads, native_op

# torch's intra-op pool follows the machine's core count, not the container's CPU quota: an oversubscribed parallel region gets
# the whole process throttled, the launching thread included (utility/host.py has the measurement)
limit_host_threads()


def _stream():
    return c_vp(torch.cuda.current_stream().cuda_stream)


def _req(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise MacaronsHipError(f"{name} must live on a HIP device (got {t.device}); "
                               "the MI355X hot path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    return t.contiguous()


def _p(t):
    return c_vp(t.data_ptr())


# ---- numerics variant of the network entry points: a property of the CALL (mcr_call_variant), scoped per thread on the host ------------
import contextlib
import threading

_tls = threading.local()


@contextlib.contextmanager
def variant(v):
    """`with ops.variant(5): ...` -- every network entry point called inside, ON THIS THREAD, runs on variant v (the one-shot per-call
    argument of the C ABI, mcr_call_variant, set before each of them).  The process default (mcr_set_local_pct_variant) is never
    touched: another thread, or another model, does not see the choice, and an exception cannot leave a flipped switch behind."""
    prev = getattr(_tls, "variant", 0)
    _tls.variant = int(v)
    try:
        yield
    finally:
        _tls.variant = prev


def current_variant():
    """The variant a network call made here and now would run on."""
    return getattr(_tls, "variant", 0) or int(lib().mcr_get_local_pct_variant())


def _net(L_):
    """Hand the scoped variant (if any) to the next network entry point of this thread; returns the library."""
    v = getattr(_tls, "variant", 0)
    if v:
        L_.mcr_call_variant(c_int(v))
    return L_


# ---- K9 scorer -------------------------------------------------------------------------------------
def _scorer_args(pts, harmonics, cams):
    pts, harmonics, cams = _req(pts, "pts"), _req(harmonics, "harmonics"), _req(cams, "X_cam")
    B, N, P = pts.shape
    C = cams.shape[1]
    if harmonics.shape != (B, N, 64):
        raise ValueError(f"harmonics must be [B,N,64] = {(B, N, 64)}, got {tuple(harmonics.shape)}")
    if cams.shape != (B, C, 3):
        raise ValueError(f"X_cam must be [B,C,3], got {tuple(cams.shape)}")
    return pts, harmonics, cams, B, N, P, C


def sh_coverage_gain(pts, harmonics, cams, use_sigmoid=True, waves_per_simd=0):
    """gains [B,C]; replaces SconeVis.compute_coverage_gain (SconeVis.py:210-252)."""
    pts, harmonics, cams, B, N, P, C = _scorer_args(pts, harmonics, cams)
    gains = torch.empty((B, C), dtype=torch.float32, device=pts.device)
    L = lib()
    ws = _workspace(pts.device, L.mcr_sh_coverage_gain_workspace_bytes(c_i64(B), c_i64(N), c_i64(C)))
    with torch.cuda.device(pts.device):
        check(L.mcr_sh_coverage_gain(_p(pts), c_int(P), _p(harmonics), _p(cams), _p(gains), c_i64(B), c_i64(N), c_i64(C),
                                     c_int(int(bool(use_sigmoid))), c_int(waves_per_simd), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_sh_coverage_gain")
    return gains


def sh_coverage_gain_best(pts, harmonics, cams, use_sigmoid=True, waves_per_simd=0):
    """(gains [B,C], record [B,2] = (max gain, first arg-max camera as fp32)): SconeVis.compute_coverage_gain (SconeVis.py:210-252) and
    the decision of testers/shapenet.py:172 (torch.max over the cameras; a NaN gain wins) in one call (mcr_sh_coverage_gain_best)."""
    pts, harmonics, cams, B, N, P, C = _scorer_args(pts, harmonics, cams)
    gains = torch.empty((B, C), dtype=torch.float32, device=pts.device)
    record = torch.empty((B, 2), dtype=torch.float32, device=pts.device)
    L = lib()
    ws = _workspace(pts.device, L.mcr_sh_coverage_gain_workspace_bytes(c_i64(B), c_i64(N), c_i64(C)))
    with torch.cuda.device(pts.device):
        check(L.mcr_sh_coverage_gain_best(_p(pts), c_int(P), _p(harmonics), _p(cams), _p(gains), _p(record), c_i64(B), c_i64(N), c_i64(C),
                                          c_int(int(bool(use_sigmoid))), c_int(waves_per_simd), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_sh_coverage_gain_best")
    return gains, record


def sh_coverage_gain_partials(pts, harmonics, cams, use_sigmoid=True, waves_per_simd=0):
    """First stage of the scorer only (sh_gain_kernel; per-(wave tile, camera) partial sums stay in the scratch arena): lets
    bench.py time the dominant kernel alone with HIP events.  Returns nothing."""
    pts, harmonics, cams, B, N, P, C = _scorer_args(pts, harmonics, cams)
    L = lib()
    ws = _entry_workspace(pts.device, L.mcr_sh_coverage_gain_workspace_bytes, c_i64(B), c_i64(N), c_i64(C))
    with torch.cuda.device(pts.device):
        check(L.mcr_sh_coverage_gain_partials(_p(pts), c_int(P), _p(harmonics), _p(cams), c_i64(B), c_i64(N), c_i64(C),
                                              c_int(int(bool(use_sigmoid))), c_int(waves_per_simd), _p(ws), c_size(ws.numel()),
                                              _stream()), "mcr_sh_coverage_gain_partials")


def sh_visibilities(pts, harmonics, cams, use_sigmoid=True):
    """vis [B,C,N]; replaces SconeVis.compute_visibilities (SconeVis.py:164-208)."""
    pts, harmonics, cams = _req(pts, "pts"), _req(harmonics, "harmonics"), _req(cams, "X_cam")
    B, N, P = pts.shape
    C = cams.shape[1]
    if harmonics.shape != (B, N, 64):
        raise ValueError(f"harmonics must be [B,N,64] = {(B, N, 64)}, got {tuple(harmonics.shape)}")
    if cams.shape != (B, C, 3):
        raise ValueError(f"X_cam must be [B,C,3], got {tuple(cams.shape)}")
    vis = torch.empty((B, C, N), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        check(lib().mcr_sh_visibilities(_p(pts), c_int(P), _p(harmonics), _p(cams), _p(vis), c_i64(B), c_i64(N),
                                        c_i64(C), c_int(int(bool(use_sigmoid))), _stream()), "mcr_sh_visibilities")
    return vis


def sh_scorer_backward(pts, harmonics, cams, grad, per_pair, use_sigmoid=True, need=(True, True, True)):
    """Gradients of sh_coverage_gain (per_pair False: grad [B,C]) or sh_visibilities (per_pair True: grad [B,C,N]) with respect to
    (harmonics, pts, cams), as (d_harm [B,N,64], d_pts [B,N,P], d_cams [B,C,3]); `need` selects which are computed (None for the
    others).  mcr_sh_scorer_backward: deterministic, HIP kernels only."""
    pts, harmonics, cams, B, N, P, C = _scorer_args(pts, harmonics, cams)
    grad = _req(grad, "grad")                       # .contiguous(): x.sum().backward() hands in an expanded, zero-stride tensor
    want = (B, C, N) if per_pair else (B, C)
    if tuple(grad.shape) != want:
        raise ValueError(f"grad must be {list(want)}, got {tuple(grad.shape)}")
    need_h, need_p, need_c = (bool(x) for x in need)
    d_harm = torch.empty((B, N, 64), dtype=torch.float32, device=pts.device) if need_h else None
    d_pts = torch.empty((B, N, P), dtype=torch.float32, device=pts.device) if need_p else None
    d_cams = torch.empty((B, C, 3), dtype=torch.float32, device=pts.device) if need_c else None
    L = lib()
    ws = _entry_workspace(pts.device, L.mcr_sh_scorer_backward_workspace_bytes, c_i64(B), c_i64(N), c_i64(C))
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    with torch.cuda.device(pts.device):
        check(L.mcr_sh_scorer_backward(_p(pts), c_int(P), _p(harmonics), _p(cams), _p(grad), c_int(int(bool(per_pair))),
                                       c_int(int(bool(use_sigmoid))), ptr(d_harm), ptr(d_pts), ptr(d_cams), c_i64(B), c_i64(N), c_i64(C),
                                       _p(ws), c_size(ws.numel()), _stream()), "mcr_sh_scorer_backward")
    return d_harm, d_pts, d_cams


# ---- K1 kNN ----------------------------------------------------------------------------------------
def knn_points(X, pc, k, subtract_query=False):
    """(pts [B,Q,k,3], dists [B,Q,k], idx [B,Q,k] int64); replaces utils.get_knn_points (utils.py:1497-1509);
    subtract_query=True also applies SconeOcc.py:297-298 (neighbours minus the query)."""
    X, pc = _req(X, "X"), _req(pc, "pc")
    B, Q, d = X.shape
    M = pc.shape[1]
    if d != 3 or pc.shape[0] != B or pc.shape[2] != 3:
        raise ValueError(f"X must be [B,Q,3] and pc [B,M,3]; got {tuple(X.shape)}, {tuple(pc.shape)}")
    idx = torch.empty((B, Q, k), dtype=torch.int64, device=X.device)
    dists = torch.empty((B, Q, k), dtype=torch.float32, device=X.device)
    pts = torch.empty((B, Q, k, 3), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        nb = int(lib().mcr_knn_grid_workspace_bytes(c_i64(B), c_i64(Q), c_i64(M)))
        ws = _workspace(X.device, nb)
        check(lib().mcr_knn_points_grid(_p(X), _p(pc), _p(idx), _p(dists), _p(pts), c_i64(B), c_i64(Q), c_i64(M), c_int(k),
                                        c_int(int(bool(subtract_query))), _p(ws), ctypes.c_size_t(ws.numel()), _stream()),
              "mcr_knn_points_grid")
    return pts, dists, idx


def knn_offsets_segmented(X, pc, cloud_sizes, query_sizes, split=True):
    """offsets [T,16,3] (neighbour minus query) of J independent k = 16 searches in one launch: job j = query rows
    sum(query_sizes[:j]) .. against cloud rows sum(cloud_sizes[:j]) ..; neighbours in knn_points' order (the ragged occupancy pass).
    split=False withholds the scratch that lets a small launch split the candidates over several workgroups (same result)."""
    X, pc = _req(X, "X"), _req(pc, "pc")
    T, J = X.shape[0], len(cloud_sizes)
    if sum(query_sizes) != T or sum(cloud_sizes) != pc.shape[0] or len(query_sizes) != J or min(cloud_sizes) < 16:
        raise ValueError("knn_offsets_segmented: sizes do not match (every cloud needs >= 16 points)")
    L = lib()
    rows = int(L.mcr_knn_rows_per_block())
    blocks, r0 = [], 0
    for j, q in enumerate(query_sizes):
        blocks += [(j, r0 + b0, min(rows, q - b0), 0) for b0 in range(0, q, rows)]
        r0 += q
    d_off = h2d(np.concatenate(([0], np.cumsum(cloud_sizes))).astype(np.int64), torch.int64, X.device)
    d_blocks = h2d(np.asarray(blocks, np.int32).reshape(-1, 4), torch.int32, X.device)
    out = torch.empty((T, 16, 3), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        ws = _entry_workspace(X.device, L.mcr_knn_offsets_segmented_workspace_bytes, c_i64(T)) if split else None
        check(L.mcr_knn_offsets_segmented(_p(X), _p(pc), _p(d_off), _p(d_blocks), c_i64(len(blocks)), c_i64(T), _p(out),
                                          _p(ws) if ws is not None else c_vp(0), c_size(ws.numel() * ws.element_size() if ws is not None else 0),
                                          _stream()), "mcr_knn_offsets_segmented")
    return out


# ---- K4/K5 building blocks ---------------------------------------------------------------------------
def _rows(t):
    """View a [..., E] tensor as rows: returns (2-D contiguous tensor, leading shape)."""
    lead = t.shape[:-1]
    return t.reshape(-1, t.shape[-1]), lead


def linear(x, weight, bias=None, gelu=False, residual=None):
    """nn.Linear (+ exact GELU) (+ residual) on the last dim; replaces Attention.py:98-103,186-188,232-235."""
    x = _req(x, "x")
    weight = _req(weight, "weight")
    x2, lead = _rows(x)
    M, K = x2.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"weight {tuple(weight.shape)} does not match input width {K}")
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    b = _req(bias, "bias") if bias is not None else None
    r = _req(residual, "residual").reshape(M, N) if residual is not None else None
    with torch.cuda.device(x.device):
        check(_net(lib()).mcr_linear(_p(x2), c_i64(K), _p(weight), _p(b) if b is not None else c_vp(0),
                               _p(r) if r is not None else c_vp(0), c_i64(N), _p(y), c_i64(N), c_i64(M), c_int(N), c_int(K),
                               c_int(int(gelu)), _stream()), "mcr_linear")
    return y.reshape(*lead, N)


def layernorm(x, weight, bias):
    x = _req(x, "x")
    x2, lead = _rows(x)
    M, E = x2.shape
    y = torch.empty_like(x2)
    with torch.cuda.device(x.device):
        check(lib().mcr_layernorm(_p(x2), c_i64(E), _p(_req(weight, "weight")), _p(_req(bias, "bias")), _p(y), c_i64(E),
                                  c_i64(M), c_int(E), _stream()), "mcr_layernorm")
    return y.reshape(*lead, E)


def _mask_bytes(mask, S, H, L, device):
    """A reference-style attention mask -> (uint8 device tensor [s, h, q, L], seq / head / query strides in bytes) for
    mcr_attention_masked.  Accepted: whatever broadcasts against the [S, H, L, L] scores the way upstream's
    `scores.masked_fill(mask == 0, -1e3)` does (Attention.py:24-27) -- [L, L], [S, 1, L, L], [1, 1, L, L], [S, H, L, L] -- plus
    [S, L, L] (the shape upstream's docstrings name: read as [S, 1, L, L]; REFUSED when S == H != 1, where upstream's broadcast
    means one mask per head instead) and key masks [S, L] (a 2-D mask of shape [L, L] is
    upstream's; use key_mask() to force the key reading when S == L) / [S, 1, 1, L].  Non-zero = attend."""
    m = mask if torch.is_tensor(mask) else torch.as_tensor(mask)
    m = (m != 0).to(device=device, dtype=torch.uint8)
    if m.dim() == 3 and tuple(m.shape) == (S, L, L) and S == H and S != 1:
        # upstream's masked_fill broadcasts [B,N,N] against [B,H,N,N] as [1,B,N,N]: with B == H that is one mask PER HEAD shared by
        # the sequences, while upstream's docstrings (and the [S,1,L,L] reading below) mean one mask per sequence -- refuse to guess
        raise ValueError(f"a 3-D attention mask of shape {tuple(m.shape)} with as many sequences as heads ({H}) is ambiguous: upstream "
                         "broadcasts it per HEAD, its docstrings mean per SEQUENCE; pass mask[:, None] ([S,1,L,L]) or mask[None] "
                         "([1,H,L,L]) explicitly")
    if m.dim() == 2 and tuple(m.shape) == (L, L):
        if S == L and S != 1:
            import warnings
            warnings.warn(f"2-D attention mask [{L}, {L}] with {S} sequences of {L} tokens: read as upstream's [L, L] pair mask; for a "
                          "[S, L] key mask use ops.key_mask()", stacklevel=3)
        m4 = m.view(1, 1, L, L)
    elif m.dim() == 2 and tuple(m.shape) == (S, L):
        m4 = m.view(S, 1, 1, L)
    elif m.dim() == 3 and tuple(m.shape) == (S, L, L):
        m4 = m.view(S, 1, L, L)
    elif m.dim() == 4 and m.shape[3] == L and m.shape[2] in (1, L) and m.shape[0] in (1, S) and m.shape[1] in (1, H):
        m4 = m
    else:
        raise ValueError(f"attention mask of shape {tuple(m.shape)} does not fit {S} sequences x {H} heads x {L} tokens")
    m4 = m4.contiguous()
    s_seq = m4.stride(0) if m4.shape[0] > 1 else 0
    s_head = m4.stride(1) if m4.shape[1] > 1 else 0
    s_q = m4.stride(2) if m4.shape[2] > 1 else 0
    return m4, s_seq, s_head, s_q


def key_mask(mask, S, L, device):
    """[S, L] key mask as the [S, 1, 1, L] form _mask_bytes takes (also when S == L)."""
    m = mask if torch.is_tensor(mask) else torch.as_tensor(mask)
    if tuple(m.shape) != (S, L):
        raise ValueError(f"key mask must be [S, L] = {(S, L)}, got {tuple(m.shape)}")
    return (m != 0).to(device=device, dtype=torch.uint8).view(S, 1, 1, L)


def attention_packed(qkv, n_heads, qk_dim, v_dim, split=True, mask=None):
    """qkv [S, L, 2*qk_dim + v_dim] -> [S, L, v_dim]; attention() + head split/merge of Attention.py:8-36,174-198.
    split=True hands the kernel a scratch buffer so that one or two long sequences can split their keys over two blocks.
    mask (optional): see _mask_bytes; masked pairs score -1e3 before the 1/sqrt(d) scale, as upstream (:24-27)."""
    qkv = _req(qkv, "qkv")
    S, L, W = qkv.shape
    if W != 2 * qk_dim + v_dim:
        raise ValueError("packed qkv width mismatch")
    out = torch.empty((S, L, v_dim), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        use_ws = split and L >= 512 and -(-L // 64) * n_heads * S <= 256      # the kernel's own key-split predicate (launch_attention)
        if mask is not None:
            m4, s_seq, s_head, s_q = _mask_bytes(mask, S, n_heads, L, qkv.device)
            ws = _workspace(qkv.device, int(lib().mcr_attention_workspace_bytes(c_i64(S), c_i64(L), c_int(n_heads), c_int(v_dim)))) if use_ws else None
            check(_net(lib()).mcr_attention_masked(_p(qkv), c_i64(W), _p(out), c_i64(v_dim), c_i64(S), c_i64(L), c_int(n_heads), c_int(qk_dim),
                                             c_int(v_dim), _p(m4), c_i64(s_seq), c_i64(s_head), c_i64(s_q),
                                             _p(ws) if ws is not None else c_vp(0), ctypes.c_size_t(ws.numel() if ws is not None else 0),
                                             _stream()), "mcr_attention_masked")
        elif use_ws:
            ws = _workspace(qkv.device, int(lib().mcr_attention_workspace_bytes(c_i64(S), c_i64(L), c_int(n_heads), c_int(v_dim))))
            check(_net(lib()).mcr_attention_ws(_p(qkv), c_i64(W), _p(out), c_i64(v_dim), c_i64(S), c_i64(L), c_int(n_heads),
                                         c_int(qk_dim), c_int(v_dim), _p(ws), ctypes.c_size_t(ws.numel()), _stream()), "mcr_attention_ws")
        else:
            check(_net(lib()).mcr_attention(_p(qkv), c_i64(W), _p(out), c_i64(v_dim), c_i64(S), c_i64(L), c_int(n_heads),
                                      c_int(qk_dim), c_int(v_dim), _stream()), "mcr_attention")
    return out


def attention_packed_planes(qkv, n_heads, qk_dim, v_dim, lens=None, split_mode=-1):
    """attention_packed on the planes pipeline of the long-sequence encoders (variant 6): the packed rows are split once into fp16 hi/lo
    planes, the kernel stages K / V tiles by LDS DMA and multiplies on fp16 pairs (attention_planes.hip).  |q|, |k|, |v| < 65504.
    lens (optional int32 [S], device): keys of sequence s = its first lens[s] rows.  split_mode: see mcr_attention_planes."""
    qkv = _req(qkv, "qkv")
    S, L, W = qkv.shape
    if W != 2 * qk_dim + v_dim:
        raise ValueError("packed qkv width mismatch")
    out = torch.empty((S, L, v_dim), dtype=torch.float32, device=qkv.device)
    if lens is not None:
        lens = _req(lens, "lens", torch.int32)
        if lens.numel() != S:
            raise ValueError("lens must hold one length per sequence")
    with torch.cuda.device(qkv.device):
        nbytes = int(lib().mcr_attention_planes_workspace_bytes(c_i64(S), c_i64(L), c_int(n_heads), c_int(qk_dim), c_int(v_dim)))
        ws = _workspace(qkv.device, nbytes)
        check(lib().mcr_attention_planes(_p(qkv), c_i64(W), _p(out), c_i64(v_dim), c_i64(S), c_i64(L), c_int(n_heads), c_int(qk_dim),
                                         c_int(v_dim), _p(lens) if lens is not None else c_vp(0), c_int(split_mode), _p(ws),
                                         ctypes.c_size_t(ws.numel()), _stream()), "mcr_attention_planes")
    return out


def colmax_broadcast(x):
    """x [S, L, E] -> [S, L, E] where every row holds the column-wise max over the L rows (Attention.py:117-121)."""
    x = _req(x, "x")
    S, L, E = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().mcr_colmax_broadcast(_p(x), c_i64(E), _p(y), c_i64(E), c_i64(S), c_i64(L), c_int(E), _stream()),
              "mcr_colmax_broadcast")
    return y


def pool_max_avg(x):
    """x [S, L, E] -> [S, 2E] = (max over L || mean over L)   (SconeOcc.py:123-126)."""
    x = _req(x, "x")
    S, L, E = x.shape
    y = torch.empty((S, 2 * E), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().mcr_pool_max_avg(_p(x), c_i64(E), _p(y), c_i64(2 * E), c_i64(S), c_i64(L), c_int(E), _stream()),
              "mcr_pool_max_avg")
    return y


# ---- network forwards ----------------------------------------------------------------------------------
_ws_cache = {}


def _workspace(device, nbytes, tag=None):
    """One grow-only scratch arena per (device, stream): the C ABI never allocates, and two streams running workspace-using ops
    concurrently must not share scratch.  A grown arena replaces the old one; the old tensor is freed by torch's caching
    allocator only after the work queued on its stream (record_stream).  `tag`: an arena of its own, for an op whose scratch has
    to survive other ops on the stream (the two-phase SconeOcc forwards keep their features in it between the calls)."""
    stream = torch.cuda.current_stream(device)
    key = (device.type, device.index, stream.cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.1) + 256, dtype=torch.uint8, device=device)
        buf.record_stream(stream)
        _ws_cache[key] = buf
    return buf


def _entry_workspace(device, size_fn, *sizes):
    """The arena, large enough for what the entry's own `size_fn(*sizes)` asks (never empty: an entry refuses a NULL workspace)."""
    return _workspace(device, max(int(size_fn(*sizes)), 4))


_ws_epoch = {}


def _bump_epoch(device, tag):
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, tag)
    _ws_epoch[key] = _ws_epoch.get(key, 0) + 1


def scone_occ_epoch(device, tag="scone_occ"):
    """How many SconeOcc launch sequences have written the tagged arena of the current stream of `device`.  The two-phase forwards
    keep phase 1's results (feature planes, query order, park counters) in that arena: a handle remembers the count after its phase 1
    and is honoured only while the count still stands (any other forward on the stream in between would have clobbered them)."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, tag)
    return _ws_epoch.get(key, 0)


def _ptr_table(tensors):
    """tensors: a list of tensors, or a (tensors, ready-made ctypes pointer array) pair from networks.packing.TableCache."""
    if isinstance(tensors, tuple):
        return tensors[1]
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def _n_weights(tensors):
    return len(tensors[0]) if isinstance(tensors, tuple) else len(tensors)


def pc_transformer_forward(pc, weights, feature_dim):
    pc = _req(pc, "pc")
    S, L, d = pc.shape
    if d != 3:
        raise ValueError("PCTransformer HIP path needs pts_dim = 3")
    L_ = lib()
    out = torch.empty((S, feature_dim), dtype=torch.float32, device=pc.device)
    nb = L_.mcr_pc_transformer_workspace_bytes(c_i64(S), c_i64(L))
    ws = _workspace(pc.device, nb)
    tab = _ptr_table(weights)
    with torch.cuda.device(pc.device):
        check(_net(L_).mcr_pc_transformer_forward(_p(pc), _p(out), c_i64(S), c_i64(L), c_int(feature_dim), tab,
                                            c_int(_n_weights(weights)), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_pc_transformer_forward")
    return out


def scone_vis_forward(pts, view_harmonics, weights, lengths=None):
    """lengths (optional, int32 device tensor [B]): cloud b = its first lengths[b] rows (padded variable-length batch)."""
    pts, view_harmonics = _req(pts, "pts"), _req(view_harmonics, "view_harmonics")
    B, N, d = pts.shape
    if d != 4 or view_harmonics.shape != (B, N, 64):
        raise ValueError(f"SconeVis HIP path needs pts [B,N,4] and view_harmonics [B,N,64]; got {tuple(pts.shape)}, "
                         f"{tuple(view_harmonics.shape)}")
    L_ = lib()
    out = torch.empty((B, N, 64), dtype=torch.float32, device=pts.device)
    nb = L_.mcr_scone_vis_workspace_bytes(c_i64(B), c_i64(N))
    ws = _workspace(pts.device, nb)
    tab = _ptr_table(weights)
    if lengths is not None:
        lengths = _req(lengths, "lengths", torch.int32).reshape(-1)
        if lengths.numel() != B:
            raise ValueError(f"lengths must hold one int32 per cloud ({B}), got {lengths.numel()}")
    with torch.cuda.device(pts.device):
        check(_net(L_).mcr_scone_vis_forward(_p(pts), _p(view_harmonics), _p(out), c_i64(B), c_i64(N), tab, c_int(_n_weights(weights)),
                                       _p(lengths) if lengths is not None else c_vp(0), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_scone_vis_forward")
    return out


def scone_vis_backward(pts, view_harmonics, d_out, weights, lengths=None, need=(True, True, True)):
    """Gradients of scone_vis_forward given d_out [B,N,64]: (d_weights, d_pts [B,N,4], d_vh [B,N,64]); `need` = (params, pts, vh)
    selects what is computed (None for the rest).  d_weights: one tensor per entry of the 48-entry weight table (table order and
    shapes; the packed qkv weight / bias one entry each).  The fp32 network's gradient whatever the variant (mcr_scone_vis_backward:
    HIP kernels only, deterministic)."""
    pts, view_harmonics = _req(pts, "pts"), _req(view_harmonics, "view_harmonics")
    d_out = _req(d_out, "d_out")                # .contiguous(): x.sum().backward() hands in an expanded, zero-stride tensor
    B, N, d = pts.shape
    if d != 4 or view_harmonics.shape != (B, N, 64) or d_out.shape != (B, N, 64):
        raise ValueError(f"SconeVis backward needs pts [B,N,4], view_harmonics and d_out [B,N,64]; got {tuple(pts.shape)}, "
                         f"{tuple(view_harmonics.shape)}, {tuple(d_out.shape)}")
    tensors = weights[0] if isinstance(weights, tuple) else weights
    need_w, need_p, need_v = (bool(x) for x in need)
    dev = pts.device
    d_w = [torch.empty(tuple(t.shape), dtype=torch.float32, device=dev) for t in tensors[:48]] if need_w else None
    d_pts = torch.empty((B, N, 4), dtype=torch.float32, device=dev) if need_p else None
    d_vh = torch.empty((B, N, 64), dtype=torch.float32, device=dev) if need_v else None
    if lengths is not None:
        lengths = _req(lengths, "lengths", torch.int32).reshape(-1)
        if lengths.numel() != B:
            raise ValueError(f"lengths must hold one int32 per cloud ({B}), got {lengths.numel()}")
    L_ = lib()
    ws = _workspace(dev, int(L_.mcr_scone_vis_backward_workspace_bytes(c_i64(B), c_i64(N))))
    dtab = (ctypes.c_void_p * 48)(*[t.data_ptr() for t in d_w]) if need_w else None
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    with torch.cuda.device(dev):
        check(L_.mcr_scone_vis_backward(_p(pts), _p(view_harmonics), _p(d_out), c_i64(B), c_i64(N), _ptr_table(weights),
                                        c_int(_n_weights(weights)), _p(lengths) if lengths is not None else c_vp(0),
                                        dtab if dtab is not None else c_vp(None), ptr(d_pts), ptr(d_vh), _p(ws), c_size(ws.numel()),
                                        _stream()), "mcr_scone_vis_backward")
    return d_w, d_pts, d_vh


def attention_backward(qkv, d_out, n_heads=4, lens=None):
    """Gradient of attention_packed (per-head widths 16 / 64; lens as attention_packed_planes) with respect to the packed rows:
    qkv [S,L,W], d_out [S,L,v_dim] -> d_qkv [S,L,W]  (mcr_attention_backward)."""
    qkv, d_out = _req(qkv, "qkv"), _req(d_out, "d_out")
    S, L, W = qkv.shape
    qk_dim, v_dim = 16 * n_heads, 64 * n_heads
    if W != 2 * qk_dim + v_dim or d_out.shape != (S, L, v_dim):
        raise ValueError(f"attention_backward: qkv [S,L,{2 * qk_dim + v_dim}] and d_out [S,L,{v_dim}] expected")
    if lens is not None:
        lens = _req(lens, "lens", torch.int32).reshape(-1)
        if lens.numel() != S:
            raise ValueError("lens must hold one length per sequence")
    d_qkv = torch.empty_like(qkv)
    L_ = lib()
    ws = _workspace(qkv.device, int(L_.mcr_attention_backward_workspace_bytes(c_i64(S), c_i64(L), c_int(n_heads), c_int(v_dim))))
    with torch.cuda.device(qkv.device):
        check(L_.mcr_attention_backward(_p(qkv), c_i64(W), _p(d_out), c_i64(v_dim), _p(d_qkv), c_i64(W), c_i64(S), c_i64(L), c_int(n_heads),
                                        c_int(qk_dim), c_int(v_dim), _p(lens) if lens is not None else c_vp(0), _p(ws), c_size(ws.numel()),
                                        _stream()), "mcr_attention_backward")
    return d_qkv


def attention_backward_pct(qkv, d_out, lens=None):
    """attention_backward at the PCTransformer's widths: 4 heads of 8 (q, k) and 32 (v), qkv [S,L,192], d_out [S,L,128] -> d_qkv
    [S,L,192] (mcr_attention_backward_pct).  L == 16: the one-wave-per-sequence kernel, any S, no lens; else S <= 65535."""
    qkv, d_out = _req(qkv, "qkv"), _req(d_out, "d_out")
    S, L, W = qkv.shape
    if W != 192 or d_out.shape != (S, L, 128):
        raise ValueError("attention_backward_pct: qkv [S,L,192] and d_out [S,L,128] expected")
    if lens is not None:
        lens = _req(lens, "lens", torch.int32).reshape(-1)
        if lens.numel() != S:
            raise ValueError("lens must hold one length per sequence")
    d_qkv = torch.empty_like(qkv)
    L_ = lib()
    ws = _workspace(qkv.device, int(L_.mcr_attention_backward_pct_workspace_bytes(c_i64(S), c_i64(L))))
    with torch.cuda.device(qkv.device):
        check(L_.mcr_attention_backward_pct(_p(qkv), c_i64(W), _p(d_out), c_i64(128), _p(d_qkv), c_i64(W), c_i64(S), c_i64(L), c_int(4),
                                            c_int(32), c_int(128), _p(lens) if lens is not None else c_vp(0), _p(ws), c_size(ws.numel()),
                                            _stream()), "mcr_attention_backward_pct")
    return d_qkv


def pool_max_avg_backward(x, d_y, lens=None):
    """Gradient of pool_max_avg: x [S,L,E], d_y [S,2E] -> d_x [S,L,E] (the max's share to the lowest row holding it).  lens (int32
    device [S], optional): padded sequences -- sequence s pools its first n = min(L, max(1, lens[s])) rows (mean divided by n), the rows
    beyond receive exact zeros (mcr_pool_max_avg_backward_lens)."""
    x, d_y = _req(x, "x"), _req(d_y, "d_y")
    S, L, E = x.shape
    if d_y.shape != (S, 2 * E):
        raise ValueError(f"pool_max_avg_backward: d_y [{S},{2 * E}] expected, got {tuple(d_y.shape)}")
    d_x = torch.empty_like(x)
    if lens is not None:
        lens = _req(lens, "lens", torch.int32).reshape(-1)
        if lens.numel() != S:
            raise ValueError("lens must hold one length per sequence")
        with torch.cuda.device(x.device):
            check(lib().mcr_pool_max_avg_backward_lens(_p(x), c_i64(E), _p(d_y), c_i64(2 * E), _p(d_x), c_i64(E), c_i64(S), c_i64(L), c_int(E),
                                                       _p(lens), _stream()), "mcr_pool_max_avg_backward_lens")
        return d_x
    with torch.cuda.device(x.device):
        check(lib().mcr_pool_max_avg_backward(_p(x), c_i64(E), _p(d_y), c_i64(2 * E), _p(d_x), c_i64(E), c_i64(S), c_i64(L), c_int(E),
                                              _stream()), "mcr_pool_max_avg_backward")
    return d_x


def pc_transformer_backward_chunk(S, L):
    """Sequences per chunk of pc_transformer_backward (mcr_pc_transformer_backward_chunk: a function of (S, L) alone)."""
    return int(lib().mcr_pc_transformer_backward_chunk(c_i64(S), c_i64(L)))


def pc_transformer_backward(pc, d_features, weights, feature_dim, need=(True, True)):
    """Gradients of pc_transformer_forward given d_features [S, feature_dim]: (d_weights, d_pc [S,L,3]); `need` = (params, pc) selects
    what is computed (None for the rest).  d_weights: one tensor per entry of the 32-entry weight table (table order and shapes; the
    packed qkv weight / bias one entry each).  The fp32 network's gradient whatever the variant (mcr_pc_transformer_backward: HIP
    kernels only, deterministic; 16-token sequences are chunked inside the entry)."""
    pc = _req(pc, "pc")
    d_features = _req(d_features, "d_features")     # .contiguous(): y.sum().backward() hands in an expanded, zero-stride tensor
    S, L, d = pc.shape
    if d != 3 or d_features.shape != (S, feature_dim):
        raise ValueError(f"PCTransformer backward needs pc [S,L,3] and d_features [S,{feature_dim}]; got {tuple(pc.shape)}, "
                         f"{tuple(d_features.shape)}")
    tensors = weights[0] if isinstance(weights, tuple) else weights
    need_w, need_p = (bool(x) for x in need)
    dev = pc.device
    d_w = [torch.empty(tuple(t.shape), dtype=torch.float32, device=dev) for t in tensors[:32]] if need_w else None
    d_pc = torch.empty((S, L, 3), dtype=torch.float32, device=dev) if need_p else None
    L_ = lib()
    ws = _workspace(dev, int(L_.mcr_pc_transformer_backward_workspace_bytes(c_i64(S), c_i64(L))))
    dtab = (ctypes.c_void_p * 32)(*[t.data_ptr() for t in d_w]) if need_w else None
    with torch.cuda.device(dev):
        check(L_.mcr_pc_transformer_backward(_p(pc), _p(d_features), c_i64(S), c_i64(L), c_int(feature_dim), _ptr_table(weights),
                                             c_int(_n_weights(weights)), dtab if dtab is not None else c_vp(None),
                                             _p(d_pc) if d_pc is not None else c_vp(None), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_pc_transformer_backward")
    return d_w, d_pc


def scone_occ_backward_chunk(Q):
    """Queries per chunk of scone_occ_backward at q_chunk=0 (mcr_scone_occ_backward_chunk: the 16-token chunk of pc_transformer_backward)."""
    return int(lib().mcr_scone_occ_backward_chunk(c_i64(Q)))


def scone_occ_backward(pc_global, pc_scales, x, view_harmonics, knn_idx, d_out, weights, need=(True, True, True), q_chunk=0):
    """Gradients of scone_occ_forward given d_out [B,Q,1] and, per scale, the neighbour indices knn_idx[i] [B,Q,16] (int64, what
    knn_points returns; no gradient flows through the selection): (d_weights, d_x [B,Q,3], d_vh [B,Q,64]); `need` = (params, x, vh)
    selects what is computed (None for the rest; nothing needed: no launch).  d_weights: one tensor per entry of the 140-entry weight
    table (table order and shapes; every transformer's packed qkv weight / bias one entry each).  There is no gradient for the
    surface points.  The fp32 network's gradient whatever the variant (mcr_scone_occ_backward: HIP kernels only, deterministic; the
    queries are processed in chunks of q_chunk rows inside the entry, 0 = scone_occ_backward_chunk(Q); the bits may depend on q_chunk)."""
    pc_global, x, view_harmonics = _req(pc_global, "pc_global"), _req(x, "x"), _req(view_harmonics, "view_harmonics")
    d_out = _req(d_out, "d_out")                # .contiguous(): y.sum().backward() hands in an expanded, zero-stride tensor
    pc_scales = [_req(p, f"pc_scales[{i}]") for i, p in enumerate(pc_scales)]
    knn_idx = [_req(t, f"knn_idx[{i}]", torch.int64) for i, t in enumerate(knn_idx)]
    B, Q, d = x.shape
    Lg = pc_global.shape[1]
    if (d != 3 or len(pc_scales) != 3 or len(knn_idx) != 3 or pc_global.shape != (B, Lg, 3) or view_harmonics.shape != (B, Q, 64)
            or d_out.numel() != B * Q or any(p.dim() != 3 or p.shape[0] != B or p.shape[2] != 3 for p in pc_scales)
            or any(t.shape != (B, Q, 16) for t in knn_idx)):
        raise ValueError("SconeOcc backward needs pc_global [B,Lg,3], three pc_scales [B,M_i,3], x [B,Q,3], view_harmonics [B,Q,64], three "
                         "knn_idx [B,Q,16] and d_out [B,Q,1]")
    tensors = weights[0] if isinstance(weights, tuple) else weights
    need_w, need_x, need_v = (bool(t) for t in need)
    if not (need_w or need_x or need_v):
        return None, None, None
    dev = x.device
    d_w = [torch.empty(tuple(t.shape), dtype=torch.float32, device=dev) for t in tensors[:140]] if need_w else None
    d_x = torch.empty((B, Q, 3), dtype=torch.float32, device=dev) if need_x else None
    d_vh = torch.empty((B, Q, 64), dtype=torch.float32, device=dev) if need_v else None
    L_ = lib()
    ws = _workspace(dev, int(L_.mcr_scone_occ_backward_workspace_bytes(c_i64(B), c_i64(Q), c_i64(Lg), c_i64(q_chunk))))
    dtab = (ctypes.c_void_p * 140)(*[t.data_ptr() for t in d_w]) if need_w else None
    sc = (ctypes.c_void_p * 3)(*[p.data_ptr() for p in pc_scales])
    ms = (ctypes.c_int64 * 3)(*[p.shape[1] for p in pc_scales])
    idx = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in knn_idx])
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    with torch.cuda.device(dev):
        check(L_.mcr_scone_occ_backward(_p(pc_global), c_i64(Lg), sc, ms, _p(x), _p(view_harmonics), idx, _p(d_out), c_i64(B), c_i64(Q),
                                        _ptr_table(weights), c_int(_n_weights(weights)), dtab if dtab is not None else c_vp(None),
                                        ptr(d_x), ptr(d_vh), c_i64(q_chunk), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_scone_occ_backward")
    return d_w, d_x, d_vh


def scone_occ_backward_ragged(pc_global, global_len, offsets, x, view_harmonics, row_job, query_sizes, d_out, weights,
                              need=(True, True, True), q_chunk=0):
    """Gradients of the ragged occupancy pass (J jobs of different sizes, scone_occ_forward_ragged) given d_out [T,1]:
    (d_weights, d_x [T,3], d_vh [T,64]), the weight gradients summed over the jobs; `need` = (params, x, vh) selects what is computed
    (None for the rest; nothing needed: no launch).  pc_global [J,Lg,3] with global_len (int32 device [J]: the valid rows of every
    padded sequence; what the padding rows hold is never used), offsets: per scale [T,16,3], neighbour minus query
    (knn_offsets_segmented; no gradient flows through the selection), x [T,3], view_harmonics [T,64], row_job (int32 device [T],
    non-decreasing), query_sizes (host list of J: job j owns the next query_sizes[j] rows; uploaded here as the J + 1 row bounds).
    The rows of all jobs are packed into chunks of q_chunk rows inside the entry (0 = scone_occ_backward_chunk(T)); a chunk may span
    any number of jobs.  The fp32 network's gradient whatever the variant (mcr_scone_occ_backward_ragged: HIP kernels only,
    deterministic; the bits may depend on q_chunk).  There is no gradient for the surface points."""
    pc_global, x, view_harmonics = _req(pc_global, "pc_global"), _req(x, "x"), _req(view_harmonics, "view_harmonics")
    d_out = _req(d_out, "d_out")
    offsets = [_req(o, f"offsets[{i}]") for i, o in enumerate(offsets)]
    global_len, row_job = _req(global_len, "global_len", torch.int32), _req(row_job, "row_job", torch.int32)
    qs = [int(q) for q in query_sizes]
    J, T = len(qs), x.shape[0]
    if (x.dim() != 2 or x.shape[1] != 3 or pc_global.dim() != 3 or pc_global.shape[0] != J or pc_global.shape[2] != 3 or len(offsets) != 3
            or any(o.shape != (T, 16, 3) for o in offsets) or view_harmonics.shape != (T, 64) or d_out.numel() != T
            or global_len.numel() != J or row_job.numel() != T or sum(qs) != T or min(qs, default=0) < 0):
        raise ValueError("SconeOcc ragged backward needs pc_global [J,Lg,3], global_len [J], three offsets [T,16,3], x [T,3], "
                         "view_harmonics [T,64], row_job [T], J query_sizes summing to T and d_out [T,1]")
    Lg = pc_global.shape[1]
    tensors = weights[0] if isinstance(weights, tuple) else weights
    need_w, need_x, need_v = (bool(t) for t in need)
    if not (need_w or need_x or need_v):
        return None, None, None
    dev = x.device
    job_rows = h2d(np.concatenate(([0], np.cumsum(qs))).astype(np.int64), torch.int64, dev)
    d_w = [torch.empty(tuple(t.shape), dtype=torch.float32, device=dev) for t in tensors[:140]] if need_w else None
    d_x = torch.empty((T, 3), dtype=torch.float32, device=dev) if need_x else None
    d_vh = torch.empty((T, 64), dtype=torch.float32, device=dev) if need_v else None
    L_ = lib()
    ws = _workspace(dev, int(L_.mcr_scone_occ_backward_ragged_workspace_bytes(c_i64(J), c_i64(T), c_i64(Lg), c_i64(q_chunk))))
    dtab = (ctypes.c_void_p * 140)(*[t.data_ptr() for t in d_w]) if need_w else None
    offs = (ctypes.c_void_p * 3)(*[o.data_ptr() for o in offsets])
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    with torch.cuda.device(dev):
        check(L_.mcr_scone_occ_backward_ragged(_p(pc_global), _p(global_len), c_i64(Lg), offs, _p(x), _p(view_harmonics), _p(row_job),
                                               _p(job_rows), _p(d_out), c_i64(J), c_i64(T), _ptr_table(weights), c_int(_n_weights(weights)),
                                               dtab if dtab is not None else c_vp(None), ptr(d_x), ptr(d_vh), c_i64(q_chunk), _p(ws),
                                               c_size(ws.numel()), _stream()), "mcr_scone_occ_backward_ragged")
    return d_w, d_x, d_vh


def linear_backward(x, weight, d_y, z=None, gelu=False, d_x=None, need=(True, True, True)):
    """Gradient of linear(x, weight, bias, gelu) given d_y: (d_x, d_w, d_b).  z: the pre-activation (needed with gelu).  d_x given:
    the input gradient is ADDED to it (in place), else a new tensor; `need` = (x, weight, bias).  mcr_linear_backward."""
    x, weight, d_y = _req(x, "x"), _req(weight, "weight"), _req(d_y, "d_y")
    x2, lead = _rows(x)
    M, K = x2.shape
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K:
        raise ValueError(f"weight {tuple(weight.shape)} does not match input width {K}")
    if d_y.numel() != M * N:
        raise ValueError(f"d_y must hold {M} x {N} values, got {tuple(d_y.shape)}")
    dy2 = d_y.reshape(M, N)
    z2 = _req(z, "z").reshape(M, N) if gelu else None
    need_x, need_w, need_b = (bool(v) for v in need)
    acc = d_x is not None
    if acc and (not d_x.is_contiguous() or d_x.dtype != torch.float32 or d_x.shape != x.shape):
        raise ValueError("d_x must be a contiguous float32 tensor shaped like x")
    dx = (d_x if acc else torch.empty_like(x2)) if need_x else None
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device) if need_w else None
    db = torch.empty((N,), dtype=torch.float32, device=x.device) if need_b else None
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    L_ = lib()
    ws = _workspace(x.device, int(L_.mcr_linear_backward_workspace_bytes(c_i64(M), c_int(N), c_int(K))))
    with torch.cuda.device(x.device):
        check(L_.mcr_linear_backward(_p(x2), c_i64(K), _p(weight), ptr(z2), c_i64(N), _p(dy2), c_i64(N), c_i64(M), c_int(N), c_int(K),
                                     c_int(int(bool(gelu))), ptr(dx), c_i64(K), c_int(int(acc)), ptr(dw), ptr(db), _p(ws), c_size(ws.numel()),
                                     _stream()), "mcr_linear_backward")
    return (dx.reshape(*lead, K) if dx is not None else None), dw, db


def layernorm_backward(x, weight, d_y, d_x=None, need=(True, True, True)):
    """Gradient of layernorm(x, weight, bias) given d_y: (d_x, d_weight, d_bias); d_x given: added to it in place."""
    x, weight, d_y = _req(x, "x"), _req(weight, "weight"), _req(d_y, "d_y")
    x2, lead = _rows(x)
    M, E = x2.shape
    acc = d_x is not None
    if acc and (not d_x.is_contiguous() or d_x.dtype != torch.float32 or d_x.shape != x.shape):
        raise ValueError("d_x must be a contiguous float32 tensor shaped like x")
    dx = d_x if acc else torch.empty_like(x2)
    need_g, need_b = bool(need[1]), bool(need[2])
    dg = torch.empty((E,), dtype=torch.float32, device=x.device) if need_g else None
    db = torch.empty((E,), dtype=torch.float32, device=x.device) if need_b else None
    ptr = lambda t: _p(t) if t is not None else c_vp(None)
    L_ = lib()
    ws = _workspace(x.device, int(L_.mcr_layernorm_backward_workspace_bytes(c_i64(M), c_int(E))))
    with torch.cuda.device(x.device):
        check(L_.mcr_layernorm_backward(_p(x2), c_i64(E), _p(weight), _p(d_y.reshape(M, E)), c_i64(E), c_i64(M), c_int(E), _p(dx), c_i64(E),
                                        c_int(int(acc)), ptr(dg), ptr(db), _p(ws), c_size(ws.numel()), _stream()), "mcr_layernorm_backward")
    return dx.reshape(*lead, E), dg, db


def colmax_backward(x, d_bcast, d_x, lens=None):
    """Gradient of the cloud-wide column max (colmax_broadcast; lens: max over the first lens[s] rows): d_x [S,L,E] += at each
    column's arg-max row (lowest on ties) the column's d_bcast summed over all L rows.  In place; returns d_x."""
    x, d_bcast = _req(x, "x"), _req(d_bcast, "d_bcast")
    S, L, E = x.shape
    if d_bcast.shape != x.shape or not d_x.is_contiguous() or d_x.shape != x.shape or d_x.dtype != torch.float32:
        raise ValueError("colmax_backward: x, d_bcast and d_x must all be [S,L,E] (d_x contiguous float32)")
    if lens is not None:
        lens = _req(lens, "lens", torch.int32).reshape(-1)
        if lens.numel() != S:
            raise ValueError(f"lens must hold one length per sequence ({S}), got {lens.numel()}")
    with torch.cuda.device(x.device):
        check(lib().mcr_colmax_backward(_p(x), c_i64(E), _p(d_bcast), c_i64(E), _p(d_x), c_i64(E), c_i64(S), c_i64(L), c_int(E),
                                        _p(lens) if lens is not None else c_vp(0), _stream()), "mcr_colmax_backward")
    return d_x


def nonfinite_flag_(x, flag):
    """flag (int32 device [1]) |= 1 if x holds an inf / NaN (mcr_nonfinite_flag); no read-back."""
    x = _req(x, "x")
    if x.numel():
        with torch.cuda.device(x.device):
            check(lib().mcr_nonfinite_flag(_p(x), c_i64(x.numel()), _p(_req(flag, "flag", torch.int32)), _stream()), "mcr_nonfinite_flag")
    return flag


def local_pct_forward(offsets, blob):
    """offsets [S,16,3] -> [S,256]: fused local PCTransformer (local_pct.hip)."""
    offsets, blob = _req(offsets, "offsets"), _req(blob, "blob")
    S = offsets.shape[0]
    if tuple(offsets.shape[1:]) != (16, 3):
        raise ValueError("offsets must be [S,16,3]")
    out = torch.empty((S, 256), dtype=torch.float32, device=offsets.device)
    with torch.cuda.device(offsets.device):
        check(_net(lib()).mcr_local_pct_forward(_p(offsets), _p(out), c_i64(256), c_i64(S), _p(blob), _stream()),
              "mcr_local_pct_forward")
    return out


def scone_occ_forward(pc_global, pc_scales, x, view_harmonics, weights, local_blobs=None, head_planes=None, range_flag=None, phase=0,
                      M_scale=None, Lg=None, out=None):
    """head_planes: packing.HeadPlaneCache.get() triple (pre-split fp16 planes of the head matrices, variant 6) or None;
    range_flag: int32 device tensor [1] the call ORs 1 into when an occupancy comes out non-finite (or None).
    phase 1 / 2 (mcr_scone_occ_forward_phase): scale 0 and the query order / the rest, as two calls on the same stream.  Phase 1
    takes pc_scales = [whole cloud, None, None] with the three sizes in M_scale and Lg, no pc_global / view_harmonics, and returns
    None; phase 2 takes everything (and `out`, if the caller already has the buffer)."""
    late = phase != 1
    x = _req(x, "x")
    B, Q = x.shape[0], x.shape[1]
    if late:
        pc_global, view_harmonics = _req(pc_global, "pc_global"), _req(view_harmonics, "view_harmonics")
        pc_scales = [_req(p, "pc_scale") for p in pc_scales]
        Lg = pc_global.shape[1]
        M_scale = [p.shape[1] for p in pc_scales]
        if pc_global.shape[0] != B or len(pc_scales) != 3 or x.shape != (B, Q, 3) or view_harmonics.shape != (B, Q, 64):
            raise ValueError("SconeOcc HIP path needs 3 scales, x [B,Q,3] and view_harmonics [B,Q,64]")
    else:
        pc_scales = [_req(pc_scales[0], "pc_scale"), None, None]
        if x.shape != (B, Q, 3) or M_scale is None or len(M_scale) != 3 or Lg is None or pc_scales[0].shape[1] != M_scale[0]:
            raise ValueError("SconeOcc phase 1 needs x [B,Q,3], the whole cloud, the three scale sizes and Lg")
    L_ = lib()
    if late and out is None:
        out = torch.empty((B, Q, 1), dtype=torch.float32, device=x.device)
    nb = L_.mcr_scone_occ_workspace_bytes(c_i64(B), c_i64(Q), c_i64(Lg))
    ws = _workspace(x.device, nb, "scone_occ")
    _bump_epoch(x.device, "scone_occ")
    tab = _ptr_table(weights)
    sc_ptrs = (ctypes.c_void_p * 3)(*[p.data_ptr() if p is not None else None for p in pc_scales])
    sc_m = (ctypes.c_int64 * 3)(*[int(m) for m in M_scale])
    blobs = (ctypes.c_void_p * 3)(*[_req(b, "local_blob").data_ptr() for b in local_blobs]) if local_blobs else None
    with torch.cuda.device(x.device):
        check(_net(L_).mcr_scone_occ_forward_phase(_p(pc_global) if late else c_vp(0), c_i64(Lg), sc_ptrs, sc_m, _p(x),
                                             _p(view_harmonics) if late else c_vp(0), _p(out) if late else c_vp(0), c_i64(B),
                                             c_i64(Q), tab, c_int(_n_weights(weights)), blobs,
                                             head_planes[1] if head_planes is not None else None,
                                             head_planes[2] if head_planes is not None else None,
                                             _p(_req(range_flag, "range_flag", torch.int32)) if range_flag is not None else c_vp(0),
                                             _p(ws), c_size(ws.numel()), c_int(int(phase)), _stream()),
              "mcr_scone_occ_forward")
    return out


def scone_occ_forward_ragged(pc_global, global_len, pc_scales, scale_offsets, x, view_harmonics, row_job, knn_blocks, weights,
                             local_blobs, head_planes=None, range_flag=None, phase=0, Lg=None, out=None, arena="scone_occ_ragged"):
    """J SconeOcc jobs of different sizes in one launch sequence (mcr_scone_occ_forward_ragged).  pc_global [J,Lg,3],
    global_len int32 [J], pc_scales: 3 ragged clouds [sum M_s,3], scale_offsets: 3 int64 [J+1], x [T,3], view_harmonics [T,64],
    row_job int32 [T], knn_blocks int32 [n_blocks,4] -> out [T,1].
    phase 1 / 2 (mcr_scone_occ_forward_ragged_phase): the part that needs no hidden draw / the rest, as two calls on the same stream
    (phase 1: pc_global / global_len may be None with Lg given, pc_scales[1:], scale_offsets[1:] are ignored; returns None)."""
    x, view_harmonics = _req(x, "x"), _req(view_harmonics, "view_harmonics")
    row_job = _req(row_job, "row_job", torch.int32)
    knn_blocks = _req(knn_blocks, "knn_blocks", torch.int32)
    late = phase != 1
    pc_scales = [_req(p, "pc_scale") for p in (pc_scales if late else [pc_scales[0]] * 3)]
    scale_offsets = [_req(o, "scale_offsets", torch.int64) for o in (scale_offsets if late else [scale_offsets[0]] * 3)]
    J = scale_offsets[0].numel() - 1
    if late:
        pc_global, global_len = _req(pc_global, "pc_global"), _req(global_len, "global_len", torch.int32)
        Lg = pc_global.shape[1]
        if pc_global.shape[0] != J or global_len.numel() != J:
            raise ValueError("scone_occ_forward_ragged: pc_global [J,Lg,3], global_len [J]")
    T = x.shape[0]
    if x.shape != (T, 3) or view_harmonics.shape != (T, 64) or row_job.numel() != T:
        raise ValueError("scone_occ_forward_ragged: x [T,3], view_harmonics [T,64], row_job [T]")
    if any(o.numel() != J + 1 for o in scale_offsets) or knn_blocks.dim() != 2 or knn_blocks.shape[1] != 4:
        raise ValueError("scone_occ_forward_ragged: scale_offsets must be [J+1], knn_blocks [n_blocks,4]")
    L_ = lib()
    if late and out is None:
        out = torch.empty((T, 1), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, L_.mcr_scone_occ_ragged_workspace_bytes(c_i64(J), c_i64(T), c_i64(Lg)), arena)
    _bump_epoch(x.device, arena)
    sc_ptrs = (ctypes.c_void_p * 3)(*[p.data_ptr() for p in pc_scales])
    off_ptrs = (ctypes.c_void_p * 3)(*[o.data_ptr() for o in scale_offsets])
    blobs = (ctypes.c_void_p * 3)(*[_req(b, "local_blob").data_ptr() for b in local_blobs])
    with torch.cuda.device(x.device):
        check(_net(L_).mcr_scone_occ_forward_ragged_phase(_p(pc_global) if late else c_vp(0), _p(global_len) if late else c_vp(0), c_i64(Lg), sc_ptrs,
                                                    off_ptrs, _p(x), _p(view_harmonics), _p(row_job), _p(knn_blocks), c_i64(knn_blocks.shape[0]),
                                                    _p(out) if late else c_vp(0), c_i64(J), c_i64(T),
                                                    _ptr_table(weights), c_int(_n_weights(weights)), blobs,
                                                    head_planes[1] if head_planes is not None else None,
                                                    head_planes[2] if head_planes is not None else None,
                                                    _p(_req(range_flag, "range_flag", torch.int32)) if range_flag is not None else c_vp(0),
                                                    _p(ws), c_size(ws.numel()), c_int(int(phase)), _stream()), "mcr_scone_occ_forward_ragged")
    return out


# ---- glue -----------------------------------------------------------------------------------
def view_state(pts, X_view, n_elev, n_azim):
    """[n_clouds, seq_len, n_elev*n_azim] fp32 0/1; replaces compute_view_state (scone_utils.py:799-860).
    X_view [n_view,3] (shared by all clouds, as the reference) or [n_clouds,n_view,3] (every cloud of a scene batch against its
    own past camera positions)."""
    pts, X_view = _req(pts, "pts"), _req(X_view, "X_view")
    B, Q, d = pts.shape
    out = torch.empty((B, Q, n_elev * n_azim), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        if X_view.dim() == 3:
            if X_view.shape[0] != B:
                raise ValueError(f"per-cloud X_view must be [n_clouds={B}, n_view, 3], got {tuple(X_view.shape)}")
            check(lib().mcr_view_state_batched(_p(pts), c_int(d), _p(X_view), _p(out), c_i64(B), c_i64(Q), c_int(X_view.shape[1]),
                                               c_int(n_elev), c_int(n_azim), c_vp(0), c_int(0), _stream()), "mcr_view_state_batched")
        else:
            check(lib().mcr_view_state(_p(pts), c_int(d), _p(X_view), _p(out), c_i64(B * Q), c_int(X_view.shape[0]), c_int(n_elev),
                                       c_int(n_azim), _stream()), "mcr_view_state")
    return out


def view_state_update_(table, rows, pts, X_view, n_elev, n_azim):
    """In place: table [P_total, n_elev*n_azim] (0/1 fp32) gets, in row rows[i], the bins of the directions from pts[i] to every
    X_view position OR'ed in: `view_states[mask] += compute_view_state(...)` followed by torch.heaviside(., 0)
    (macarons_utils.py:2867-2877) as one launch.  rows: int64 device tensor [n] (None: row i <- point i)."""
    table, pts, X_view = _req(table, "view_states"), _req(pts, "pts"), _req(X_view, "X_view")
    n, d = pts.shape
    if table.shape[-1] != n_elev * n_azim:
        raise ValueError("view-state table width does not match the lattice")
    if n == 0:
        return table
    r = _req(rows, "rows", torch.int64) if rows is not None else None
    if r is not None and r.numel() != n:
        raise ValueError("rows must hold one table row per point")
    with torch.cuda.device(pts.device):
        check(lib().mcr_view_state_batched(_p(pts), c_int(d), _p(X_view), _p(table), c_i64(1), c_i64(n), c_int(X_view.shape[0]),
                                           c_int(n_elev), c_int(n_azim), _p(r) if r is not None else c_vp(0), c_int(1), _stream()),
              "mcr_view_state_batched")
    return table


def transform_points_batched_(pts, M_view, center, inv_diag, cloud_of=None):
    """In place, all clouds in one launch: pts [K,S,d] (or, with cloud_of int32 [n], ragged rows [n,d]); M_view [K,4,4],
    center [K,3], inv_diag [K]:  pts[..., :3] <- (([x y z 1] M_view[c])[:3] - center[c]) * inv_diag[c]."""
    pts = _req(pts, "pts")
    M_view, center, inv_diag = _req(M_view, "M_view"), _req(center, "center"), _req(inv_diag, "inv_diag")
    K = M_view.shape[0]
    d = pts.shape[-1]
    if cloud_of is not None:
        cloud_of = _req(cloud_of, "cloud_of", torch.int32)
        n, per = pts.shape[0], 0
    else:
        n, per = 0, pts.shape[1]
        if pts.shape[0] != K:
            raise ValueError("transform_points_batched_: one matrix per cloud")
    if pts.numel() == 0:
        return pts
    with torch.cuda.device(pts.device):
        check(lib().mcr_transform_points_batched(_p(pts), c_int(d), c_i64(K), c_i64(per), _p(M_view), _p(center), _p(inv_diag),
                                                 _p(cloud_of) if cloud_of is not None else c_vp(0), c_i64(n), _stream()),
              "mcr_transform_points_batched")
    return pts


def sample_proxy_batched(X, preds, view_harmonics, u, min_occ):
    """B clouds at once, no host sync: X [B,P,3], preds [B,P], view_harmonics [B,P,64] or None, u [B,n] ->
    (res [B,n,4], res_harmonics [B,n,64] | None, inverse [B,n] int64, uniq [B,n] int64, n_unique int32 [B], volume fp64 [B]);
    rows beyond n_unique[b] are zero.  Cloud b is sampled exactly as sample_proxy(X[b], preds[b], ...) would."""
    X, preds, u = _req(X, "X"), _req(preds, "preds"), _req(u, "samples")
    vh = _req(view_harmonics, "view_harmonics") if view_harmonics is not None else None
    shared = X.dim() == 2                          # X [P,3] / view_harmonics [P,64] common to the B distributions (preds [B,P])
    B, P = (preds.shape[0], X.shape[0]) if shared else (X.shape[0], X.shape[1])
    n = u.shape[-1]
    if preds.numel() != B * P or u.numel() != B * n:
        raise ValueError("sample_proxy_batched: preds must be [B,P] and samples [B,n]")
    dev = X.device
    res = torch.empty((B, n, 4), dtype=torch.float32, device=dev)
    resh = torch.empty((B, n, 64), dtype=torch.float32, device=dev) if vh is not None else None
    uniq = torch.empty((B, n), dtype=torch.int64, device=dev)
    inv = torch.empty((B, n), dtype=torch.int64, device=dev)
    nu = torch.empty(B, dtype=torch.int32, device=dev)
    vol = torch.empty(B, dtype=torch.float64, device=dev)
    L_ = lib()
    ws = _workspace(dev, L_.mcr_sample_proxy_batched_workspace_bytes(c_i64(B), c_i64(P), c_int(n)))
    with torch.cuda.device(dev):
        fn = L_.mcr_sample_proxy_shared if shared else L_.mcr_sample_proxy_batched
        check(fn(_p(X), _p(preds), c_i64(1), _p(vh) if vh is not None else c_vp(0), c_i64(B), c_i64(P),
                                          c_f32(float(min_occ)), _p(u), c_int(n), _p(res), _p(resh) if resh is not None else c_vp(0),
                                          _p(uniq), _p(inv), _p(nu), _p(vol), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_sample_proxy_batched")
    return res, resh, inv, uniq, nu, vol


def sample_proxy(X, preds, view_harmonics, u, min_occ, return_volume=False, padded=False):
    """(res [n_u,4], res_harmonics [n_u,64], inverse [n_sample] int64, unique original indices [n_u] int64[, volume]);
    replaces sample_proxy_points (scone_utils.py:1030-1061).  One host sync to read n_u (torch.unique syncs too) -- unless
    padded=True: then res / res_harmonics / uniq keep their n_sample rows (zeros beyond n_u) and the count comes back as an
    int32 device tensor [1] in place of the slicing: (res, res_harmonics, inverse, uniq, n_unique[, volume]), no host sync."""
    X, preds, u = _req(X, "X"), _req(preds, "preds"), _req(u, "samples")
    vh = _req(view_harmonics, "view_harmonics") if view_harmonics is not None else None    # None: res_harmonics comes back as None
    P = X.shape[0]
    n = u.numel()
    dev = X.device
    res = torch.empty((n, 4), dtype=torch.float32, device=dev)
    resh = torch.empty((n, 64), dtype=torch.float32, device=dev) if vh is not None else None
    uniq = torch.empty(n, dtype=torch.int64, device=dev)
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    nu = torch.zeros(1, dtype=torch.int32, device=dev)
    vol = torch.zeros(1, dtype=torch.float64, device=dev)
    L_ = lib()
    ws = _workspace(dev, L_.mcr_sample_proxy_workspace_bytes(c_i64(P), c_int(n)))
    with torch.cuda.device(dev):
        check(L_.mcr_sample_proxy(_p(X), _p(preds), c_i64(1), _p(vh) if vh is not None else c_vp(0), c_i64(P),
                                  c_f32(float(min_occ)), _p(u), c_int(n), _p(res), _p(resh) if resh is not None else c_vp(0),
                                  _p(uniq), _p(inv), _p(nu), _p(vol), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_sample_proxy")
    if padded:
        return (res, resh, inv, uniq, nu, vol) if return_volume else (res, resh, inv, uniq, nu)
    k = int(nu.item())
    if return_volume:
        return res[:k], resh[:k], inv, uniq[:k], vol
    return res[:k], resh[:k], inv, uniq[:k]


def points_in_fov(pts, cameras):
    """pts [P,3], cameras [n_cam,40] (layout in include/macarons_hip.h) -> bool mask [n_cam,P];
    replaces Camera.get_points_in_fov (macarons_utils.py:2400-2435)."""
    pts, cameras = _req(pts, "pts"), _req(cameras, "cameras")
    P, C = pts.shape[0], cameras.shape[0]
    if cameras.shape[1] != 40 or pts.shape[1] != 3:
        raise ValueError("cameras must be [n_cam,40] and pts [P,3]")
    mask = torch.empty((C, P), dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        check(lib().mcr_points_in_fov(_p(pts), c_i64(P), _p(cameras), c_int(C), _p(mask), _stream()), "mcr_points_in_fov")
    return mask.bool()


def coverage_gain_multiple(pts, harmonics, cams, n_cam, use_sigmoid=True):
    """(gains [B, C^n], idx [C^n, n]); replaces SconeVis.compute_coverage_gain_multiple (SconeVis.py:254-303)."""
    vis = sh_visibilities(pts, harmonics, cams, use_sigmoid)
    B, C, N = vis.shape
    out = torch.empty((B, C ** n_cam), dtype=torch.float32, device=vis.device)
    with torch.cuda.device(vis.device):
        check(lib().mcr_coverage_gain_multiple(_p(vis), _p(out), c_i64(B), c_i64(C), c_i64(N), c_int(n_cam), _stream()),
              "mcr_coverage_gain_multiple")
    single = torch.arange(0, C)
    n_idx = torch.cartesian_prod(*([single] * n_cam))                  # SconeVis.py:292-296 (index table, host)
    return out, n_idx


_pinned_pool = {}        # (device index) -> list of [pinned uint8 buffer, event of its last copy]


def _native_h2d():
    """Is torch.ops.macarons.h2d there (the C++ extension built)?  MCR_NATIVE_H2D=0: the Python restatement below (A/B)."""
    return native_op("h2d", "MCR_NATIVE_H2D")      # (read from os.environ there, once)


def h2d(data, dtype, device):
    """Host data (list / numpy array / CPU tensor) -> device tensor WITHOUT stalling the host: a `.to(device)` from pageable memory
    is a stream-ordered blocking copy, i.e. the host waits for every kernel queued before it (the glue of a MACARONS decision did
    that ~15 times per decision).  The data is staged in a small pool of re-used pinned buffers (power-of-two sizes; a buffer is
    taken again once the event behind its last copy has fired) and copied asynchronously.  (torch's own pin_memory() allocates a
    new pinned block for every new size: 80 ms for the 1 MB index array of a ragged occupancy pass.)"""
    t = data if torch.is_tensor(data) else torch.as_tensor(data)
    t = t.to(dtype) if t.dtype != dtype else t
    device = torch.device(device)
    if device.type != "cuda" or t.device.type != "cpu":
        return t.to(device)
    if _native_h2d():                                   # the same steps from C++ (libmacarons_torch.so): one dispatcher call
        return torch.ops.macarons.h2d(t, device.index if device.index is not None else torch.cuda.current_device())
    t = t.contiguous()
    nbytes = t.numel() * t.element_size()
    if nbytes == 0:
        return torch.empty(t.shape, dtype=dtype, device=device)
    pool = _pinned_pool.setdefault(device.index if device.index is not None else torch.cuda.current_device(), [])
    slot = None
    for ent in pool:
        if ent[0].numel() >= nbytes and (slot is None or ent[0].numel() < slot[0].numel()) and ent[1].query():
            slot = ent
    if slot is None:
        cap = 1 << max(12, (nbytes - 1).bit_length())
        slot = [torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
        pool.append(slot)
    stage = slot[0][:nbytes].view(dtype).view(t.shape)
    stage.copy_(t)
    with torch.cuda.device(device):
        out = stage.to(device, non_blocking=True)
        slot[1].record(torch.cuda.current_stream(device))
    return out


def gather_columns(x, idx):
    """x [..., V] fp32, idx [V] integer (values in [0, V)) -> x[..., idx] (torch.gather along the last dim with one index row).
    A host idx is range-checked on the host and uploaded without a stall; a device idx is trusted (checking it would read it
    back)."""
    x = _req(x, "x")
    V = x.shape[-1]
    if idx.device.type == "cpu":
        if idx.numel() != V or int(idx.min()) < 0 or int(idx.max()) >= V:
            raise ValueError("gather_columns: idx must hold V indices in [0, V)")
        idx = h2d(idx, torch.int32, x.device)
    else:
        if idx.numel() != V:
            raise ValueError("gather_columns: idx must hold V indices in [0, V)")
        idx = idx.to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().mcr_gather_columns(_p(x), _p(idx), _p(out), c_i64(x.numel() // V), c_int(V), _stream()), "mcr_gather_columns")
    return out


def filter_proxy_mask(X, pc, proj, filter_tol):
    """X [P,3], pc [M,3], proj [n_view,4,4] (row-vector full-projection matrices) -> (mask bool [P], bounds [n_view,4])."""
    X, pc, proj = _req(X, "X"), _req(pc, "pc"), _req(proj, "proj")
    if X.dim() != 2 or pc.dim() != 2 or X.shape[1] != 3 or pc.shape[1] != 3:
        raise NameError("Wrong shapes! X must have shape (n_proxy_points, 3) and pc must have shape (N, 3).")
    n_view = proj.shape[0]
    if tuple(proj.shape[1:]) != (4, 4):
        raise ValueError("proj must be [n_view,4,4]")
    mask = torch.empty(X.shape[0], dtype=torch.uint8, device=X.device)
    bounds = torch.empty((n_view, 4), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        check(lib().mcr_filter_proxy_points(_p(X), c_i64(X.shape[0]), _p(pc), c_i64(pc.shape[0]), _p(proj), c_int(n_view),
                                            c_f32(float(filter_tol)), _p(bounds), _p(mask), _stream()), "mcr_filter_proxy_points")
    return mask.bool(), bounds


def best_record(gains, idx_offset=0, out=None):
    """gains [B,C] -> records [B,2] fp32 = (max, idx_offset + first arg-max): torch.max(gains, dim=1) as one 8-byte record."""
    gains = _req(gains, "gains")
    B, C = gains.shape
    if out is None:
        out = torch.empty((B, 2), dtype=torch.float32, device=gains.device)
    with torch.cuda.device(gains.device):
        check(lib().mcr_best_record(_p(gains), c_i64(B), c_i64(C), c_i64(int(idx_offset)), _p(out), _stream()), "mcr_best_record")
    return out


def nbv_decide(gains, n_unique=None, range_flag=None):
    """gains [B,C] (modified in place: NaN rows where n_unique < 1) -> (max_gain [B], nbv_idx [B] int64, record float64 [1 + 2B] =
    (range flag, indices, maxima)); mcr_nbv_decide."""
    gains = _req(gains, "gains")
    B, C = gains.shape
    dev = gains.device
    max_gain = torch.empty(B, dtype=torch.float32, device=dev)
    nbv_idx = torch.empty(B, dtype=torch.int64, device=dev)
    record = torch.empty(1 + 2 * B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().mcr_nbv_decide(_p(gains), c_i64(B), c_i64(C),
                                   _p(_req(n_unique, "n_unique", torch.int32)) if n_unique is not None else c_vp(0),
                                   _p(_req(range_flag, "range_flag", torch.int32)) if range_flag is not None else c_vp(0),
                                   _p(max_gain), _p(nbv_idx), _p(record), _stream()), "mcr_nbv_decide")
    return max_gain, nbv_idx, record


def best_merge(records, out_vals=None, out_idx=None):
    """records [world,B,2] -> (vals [B] fp32, idx [B] int64) of the global arg-max, ties to the lowest index."""
    records = _req(records, "records")
    world, B = records.shape[0], records.shape[1]
    vals = out_vals if out_vals is not None else torch.empty(B, dtype=torch.float32, device=records.device)
    idx = out_idx if out_idx is not None else torch.empty(B, dtype=torch.int64, device=records.device)
    with torch.cuda.device(records.device):
        check(lib().mcr_best_merge(_p(records), c_int(world), c_i64(B), _p(vals), _p(idx), _stream()), "mcr_best_merge")
    return vals, idx


def fov_mask_occ(mask, occ):
    """mask [n_cam,P] bool/uint8, occ [P] -> [n_cam,P] occupancy zeroed outside each frustum."""
    occ = _req(occ, "occ")
    m = mask.to(torch.uint8).contiguous()
    C, P = m.shape
    out = torch.empty((C, P), dtype=torch.float32, device=occ.device)
    with torch.cuda.device(occ.device):
        check(lib().mcr_fov_mask_occ(_p(m), _p(occ), c_i64(1), _p(out), c_i64(P), c_int(C), _stream()), "mcr_fov_mask_occ")
    return out


def transform_points_(pts, M_view, center, inv_diag):
    """In place: pts[:, :3] <- (([x y z 1] M_view)[:3] - center) * inv_diag."""
    pts = _req(pts, "pts")
    n, d = pts.shape
    with torch.cuda.device(pts.device):
        check(lib().mcr_transform_points(_p(pts), c_int(d), c_i64(n), _p(_req(M_view, "M_view")), _p(_req(center, "center")),
                                         c_f32(float(inv_diag)), _stream()), "mcr_transform_points")
    return pts


def macarons_gain_(vis, pts_world, cam_world, volume, distance_th, smooth=False):
    """vis [B,N] (scaled in place by the distance factor), pts_world [B,N,>=3], cam_world [B,3], volume [B] -> gains [B].
    smooth=False: min(1, (th/d)^2); smooth=True: 1/(1+(d/th)^2)."""
    vis, pts_world, cam_world, volume = _req(vis, "vis"), _req(pts_world, "pts_world"), _req(cam_world, "cam_world"), _req(volume, "volume")
    B, N = vis.shape
    gains = torch.empty(B, dtype=torch.float32, device=vis.device)
    with torch.cuda.device(vis.device):
        check(lib().mcr_macarons_gain(_p(vis), _p(pts_world), c_int(pts_world.shape[-1]), _p(cam_world), _p(volume),
                                      c_f32(float(distance_th)), c_int(int(bool(smooth))), c_i64(B), c_i64(N), _p(gains), _stream()),
              "mcr_macarons_gain")
    return gains


# ---- scene-side bookkeeping ---------------------------------------------------------------
def min_dist_segmented(A, a_offsets, B, b_offsets, max_a=None):
    """fp64 distance of every A point to the nearest B point of its segment (grid cell); +inf for empty B segments.
    Replaces torch.min(torch.cdist(a.double(), b.double())) (macarons_utils.py:2566, 3022, 3049)."""
    A, B = _req(A, "A"), _req(B, "B")
    a_off = _req(a_offsets, "a_offsets", torch.int64)
    b_off = _req(b_offsets, "b_offsets", torch.int64)
    nseg = a_off.numel() - 1
    out = torch.empty(A.shape[0], dtype=torch.float64, device=A.device)
    if max_a is None:                                 # (an upper bound of the largest A segment avoids this read-back: it only sizes the grid)
        max_a = int((a_off[1:] - a_off[:-1]).max().item()) if nseg > 0 else 0
    if max_a == 0 or A.shape[0] == 0:
        return out
    if B.shape[0] == 0:                                  # every segment's B is empty
        return out.fill_(float("inf"))
    with torch.cuda.device(A.device):
        check(lib().mcr_min_dist_segmented(_p(A), _p(a_off), _p(B), _p(b_off), c_i64(nseg), c_i64(max_a), _p(out), _stream()),
              "mcr_min_dist_segmented")
    return out


def unproject_depth(depth, cameras):
    """depth [n_cam,H,W(,1)], cameras [n_cam,18] (Minv[16], k22, k32) -> world points [n_cam, H*W, 3]."""
    depth, cameras = _req(depth, "depth"), _req(cameras, "cameras")
    n, H, W = depth.shape[0], depth.shape[1], depth.shape[2]
    out = torch.empty((n, H * W, 3), dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        check(lib().mcr_unproject_depth(_p(depth), c_int(H), c_int(W), _p(cameras), c_i64(n), _p(out), _stream()),
              "mcr_unproject_depth")
    return out


def signed_distance_to_depth(pts, camera, depth, mask=None, fill=0.0):
    """pts [n,3], camera: >= 32 floats (M_view[16] | M_full_projection[16], the head of a points_in_fov record), depth [H,W],
    mask [H,W] bool/uint8 or None -> signed distances [n]; replaces Camera.get_signed_distance_to_depth_maps
    (macarons_utils.py:2451-2500) for one camera (pixels outside the mask count as `fill` = 1.1 zfar)."""
    pts, camera, depth = _req(pts, "pts"), _req(camera, "camera"), _req(depth, "depth")
    H, W = depth.shape[-2], depth.shape[-1]
    n = pts.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    m = mask.to(torch.uint8).contiguous() if mask is not None else None
    with torch.cuda.device(pts.device):
        check(lib().mcr_signed_distance_to_depth(_p(pts), c_i64(n), _p(camera), _p(depth), _p(m) if m is not None else c_vp(0),
                                                 c_int(H), c_int(W), c_f32(float(fill)), _p(out), _stream()),
              "mcr_signed_distance_to_depth")
    return out


def proxy_scene_update_(proxy_points, fov_mask, camera, depth, depth_mask, fill, X_cam, distance_to_surface, tol, score_threshold,
                        n_elev, n_azim, view_states, n_inside, n_behind, supervision_occ, out_of_field, return_sgn=False):
    """The proxy-point bookkeeping of one MACARONS step (testers/scene.py:402-418) fused in one pass, in place on the state
    tensors (see mcr_proxy_scene_update).  fov_mask [P] bool/uint8; returns the signed distances [P] if asked (0 outside the mask)."""
    pp = _req(proxy_points, "proxy_points")
    P = pp.shape[0]
    fm = fov_mask.to(torch.uint8).contiguous()
    dm = depth_mask.to(torch.uint8).contiguous() if depth_mask is not None else None
    depth = _req(depth, "depth")
    H, W = depth.shape[-2], depth.shape[-1]
    for name, t in (("view_states", view_states), ("n_inside", n_inside), ("n_behind", n_behind), ("supervision_occ", supervision_occ),
                    ("out_of_field", out_of_field)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 device tensor (updated in place)")
    sgn = torch.zeros(P, dtype=torch.float32, device=pp.device) if return_sgn else None
    with torch.cuda.device(pp.device):
        check(lib().mcr_proxy_scene_update(_p(pp), c_i64(P), _p(fm), _p(_req(camera, "camera")), _p(depth),
                                           _p(dm) if dm is not None else c_vp(0), c_int(H), c_int(W), c_f32(float(fill)),
                                           _p(_req(X_cam, "X_cam")), c_f32(float(distance_to_surface)), c_f32(float(tol)),
                                           c_f32(float(score_threshold)), c_int(n_elev), c_int(n_azim), _p(view_states), _p(n_inside),
                                           _p(n_behind), _p(supervision_occ), _p(out_of_field), _p(sgn) if sgn is not None else c_vp(0),
                                           _stream()), "mcr_proxy_scene_update")
    return sgn


def _check_n_frames(K, what):
    if not 1 <= K <= 32:
        raise ValueError(f"{what}: between 1 and 32 frames (one bit of fov_bits each), got {K}")


def supervision_frames(proxy_points, cameras, depth, depth_mask, fill, surface_distance):
    """The supervision signal of K new depth frames over the proxy points (train_macarons.py:386-415) in one pass
    (mcr_supervision_frames): proxy_points [P,3], cameras [K,40], depth [K,H,W], depth_mask [K,H,W] bool/uint8 or None, fill: K host
    numbers (1.1 zfar) -> fov_bits [P] int32 (bit k = in frustum k), sgn [K,P] (0 where the bit is clear), close [P] bool (upstream's
    overwrite rule: the last frame whose frustum holds the point decides)."""
    K = int(cameras.shape[0])
    _check_n_frames(K, "supervision_frames")
    pp, cams, depth = _req(proxy_points, "proxy_points"), _req(cameras, "cameras"), _req(depth, "depth")
    if cams.shape[1] != 40 or pp.shape[1] != 3:
        raise ValueError("cameras must be [K,40] and proxy_points [P,3]")
    P, H, W = pp.shape[0], depth.shape[-2], depth.shape[-1]
    if depth.numel() != K * H * W:
        raise ValueError(f"depth must hold K = {K} maps, got {tuple(depth.shape)}")
    dm = None
    if depth_mask is not None:
        dm = depth_mask.to(torch.uint8).contiguous()
        if dm.numel() != K * H * W:
            raise ValueError(f"depth_mask must hold K = {K} maps, got {tuple(depth_mask.shape)}")
    fills = (ctypes.c_float * K)(*[float(f) for f in fill])
    bits = torch.empty(P, dtype=torch.int32, device=pp.device)
    sgn = torch.empty((K, P), dtype=torch.float32, device=pp.device)
    close = torch.empty(P, dtype=torch.uint8, device=pp.device)
    if P == 0:
        return bits, sgn, close.bool()
    with torch.cuda.device(pp.device):
        check(lib().mcr_supervision_frames(_p(pp), c_i64(P), _p(cams), c_int(K), _p(depth), _p(dm) if dm is not None else c_vp(0),
                                           c_int(H), c_int(W), fills, c_f32(float(surface_distance)), _p(bits), _p(sgn), _p(close),
                                           _stream()), "mcr_supervision_frames")
    return bits, sgn, close.bool()


def proxy_scene_update_frames_(proxy_points, fov_bits, sgn, X_cam, distance_to_surface, tol, score_threshold, n_elev, n_azim,
                               view_states, n_inside, n_behind, supervision_occ, out_of_field):
    """K successive proxy_scene_update_ calls from the bits and distances of supervision_frames, in place on the state tensors
    (mcr_proxy_scene_update_frames; train_macarons.py:476-487).  sgn [K,P], X_cam [K,3]."""
    K = int(sgn.shape[0])
    _check_n_frames(K, "proxy_scene_update_frames_")
    pp, sgn, xc = _req(proxy_points, "proxy_points"), _req(sgn, "sgn"), _req(X_cam, "X_cam")
    bits = _req(fov_bits, "fov_bits", torch.int32)
    P = pp.shape[0]
    if sgn.shape[1] != P or bits.numel() != P or xc.numel() != 3 * K:
        raise ValueError("fov_bits must be [P], sgn [K,P] and X_cam [K,3]")
    for name, t in (("view_states", view_states), ("n_inside", n_inside), ("n_behind", n_behind), ("supervision_occ", supervision_occ),
                    ("out_of_field", out_of_field)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous fp32 device tensor (updated in place)")
    if view_states.numel() != P * n_elev * n_azim or any(t.numel() != P for t in (n_inside, n_behind, supervision_occ, out_of_field)):
        raise ValueError("the state tensors must hold one row per proxy point")
    if P == 0:
        return
    with torch.cuda.device(pp.device):
        check(lib().mcr_proxy_scene_update_frames(_p(pp), c_i64(P), _p(bits), _p(sgn), c_int(K), _p(xc), c_f32(float(distance_to_surface)),
                                                  c_f32(float(tol)), c_f32(float(score_threshold)), c_int(n_elev), c_int(n_azim),
                                                  _p(view_states), _p(n_inside), _p(n_behind), _p(supervision_occ), _p(out_of_field),
                                                  _stream()), "mcr_proxy_scene_update_frames")


# ---- scene-grid bookkeeping, fused (Scene.fill_cells / the cell lookup of the occupancy field) -----------------------------------------
def cell_keys(pts, grid_consts, grid, lo_tab=None, hi_tab=None, valid=None):
    """pts [N,3] -> int32 [N]: linear id of the cell each point falls in (upstream's floor rule); with the cells' bounds lo_tab / hi_tab
    [n_cells,3] also Cell.fill's tests: n_cells for a point outside the scene box, not strictly inside its cell, or with valid[i] == 0.
    grid_consts: fp32 device tensor [9] = x_min, x_max, step; grid = (grid_l, grid_w, grid_h)."""
    pts, gc = _req(pts, "pts"), _req(grid_consts, "grid_consts")
    N = pts.shape[0]
    key = torch.empty(N, dtype=torch.int32, device=pts.device)
    if N == 0:
        return key
    box = lo_tab is not None
    v = valid.to(torch.uint8).contiguous() if valid is not None else None
    with torch.cuda.device(pts.device):
        check(lib().mcr_cell_keys(_p(pts), c_i64(N), _p(v) if v is not None else c_vp(0), _p(gc), c_int(grid[0]), c_int(grid[1]), c_int(grid[2]),
                                  _p(_req(lo_tab, "lo_tab")) if box else c_vp(0), _p(_req(hi_tab, "hi_tab")) if box else c_vp(0),
                                  c_int(int(box)), _p(key), _stream()), "mcr_cell_keys")
    return key


def key_histogram(key, nk):
    """key int32 [N] -> (counts int64 [nk+1], exclusive offsets int64 [nk+2])."""
    key = _req(key, "key", torch.int32)
    if nk > 1023:                                   # grids beyond the one-block kernel's LDS table (> 1023 cells): device ops, same result
        counts = torch.zeros(nk + 1, dtype=torch.int64, device=key.device).scatter_add_(0, key.long().clamp_(0, nk), torch.ones_like(key, dtype=torch.int64))
        offsets = torch.zeros(nk + 2, dtype=torch.int64, device=key.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return counts, offsets
    counts = torch.empty(nk + 1, dtype=torch.int64, device=key.device)
    offsets = torch.empty(nk + 2, dtype=torch.int64, device=key.device)
    with torch.cuda.device(key.device):
        check(lib().mcr_key_histogram(_p(key), c_i64(key.numel()), c_int(nk), _p(counts), _p(offsets), _stream()), "mcr_key_histogram")
    return counts, offsets


def admit_keys(d, key_s, cand, resolution, n_point_min, nk):
    """Cell.fill's admission on the sorted candidates (mcr_admit_keys) -> key2 int32 [N]."""
    d, key_s, cand = _req(d, "d", torch.float64), _req(key_s, "key_s", torch.int32), _req(cand, "cand", torch.int64)
    key2 = torch.empty_like(key_s)
    if key_s.numel() == 0:
        return key2
    with torch.cuda.device(d.device):
        check(lib().mcr_admit_keys(_p(d), _p(key_s), _p(cand), c_i64(key_s.numel()), ctypes.c_double(float(resolution)), c_i64(int(n_point_min)),
                                   c_int(nk), _p(key2), _stream()), "mcr_admit_keys")
    return key2


# ---- one MACARONS decision without the host glue (scene.hip): each phase = a handful of launches behind one C call ----------------
def group_by_key(key, nk):
    """key int32 [N] in 0 .. nk (anything else counts as nk) -> (order int32 [N] = torch.sort(key, stable=True).indices,
    counts int64 [nk+1], exclusive offsets int64 [nk+2]); a three-launch counting sort (nk <= 1023)."""
    key = _req(key, "key", torch.int32)
    N, dev = key.numel(), key.device
    order = torch.empty(N, dtype=torch.int32, device=dev)
    co = torch.empty(2 * nk + 3, dtype=torch.int64, device=dev)
    L_ = lib()
    ws = _entry_workspace(dev, L_.mcr_group_by_key_workspace_bytes, c_i64(N), c_int(nk))
    with torch.cuda.device(dev):
        check(L_.mcr_group_by_key(_p(key), c_i64(N), c_int(nk), _p(order), _p(co), c_vp(co.data_ptr() + 8 * (nk + 1)), _p(ws),
                                  c_size(ws.numel()), _stream()), "mcr_group_by_key")
    return order, co[:nk + 1], co[nk + 1:]


class PendingFill:
    """What mcr_scene_fill_begin left on the device: the candidates grouped by cell and the admitted ones among them; `counts`
    (int64 [4 nk + 7] = cand | a_off | adm | adm_off | n_ambiguous) is what the host reads back before it draws the cells' permutations;
    n_ambiguous > 0: some offered point lies strictly inside a cell other than its floor cell, where upstream's rule (every englobing
    cell tests every point) and the fused one may part -- the caller fills upstream's way (Scene.fill_cells)."""
    __slots__ = ("pts", "features", "N", "nk", "key", "order", "dmin", "key2", "order2", "counts")


def scene_fill_begin(pts, valid, grid_consts, grid, lo_tab, hi_tab, store_pts, store_off, resolution, n_point_min, features=None):
    """The device part of Scene.fill_cells (mcr_scene_fill_begin): nothing returns to the host.  pts [N,3]; valid bool/uint8 [N] or
    None; store_pts [n_store,3] = every cell's stored points (cells in linear order), store_off int64 device [n_cells+1]."""
    pts, gc = _req(pts, "pts"), _req(grid_consts, "grid_consts")
    N, dev = pts.shape[0], pts.device
    nk = grid[0] * grid[1] * grid[2]
    h = PendingFill()
    h.pts, h.N, h.nk = pts, N, nk
    h.features = None if features is None else features.to(torch.float32).contiguous()
    ib = torch.empty(4 * N, dtype=torch.int32, device=dev)
    h.key, h.order, h.key2, h.order2 = ib[:N], ib[N:2 * N], ib[2 * N:3 * N], ib[3 * N:]
    h.dmin = torch.empty(N, dtype=torch.float64, device=dev)
    h.counts = torch.empty(4 * nk + 7, dtype=torch.int64, device=dev)
    v = valid.to(torch.uint8).contiguous() if valid is not None else None
    L_ = lib()
    ws = _entry_workspace(dev, L_.mcr_scene_fill_workspace_bytes, c_i64(N), c_int(nk))
    with torch.cuda.device(dev):
        check(L_.mcr_scene_fill_begin(_p(pts), c_i64(N), _p(v) if v is not None else c_vp(0), _p(gc), c_int(grid[0]), c_int(grid[1]),
                                      c_int(grid[2]), _p(_req(lo_tab, "lo_tab")), _p(_req(hi_tab, "hi_tab")),
                                      _p(store_pts) if store_pts is not None and store_pts.numel() else c_vp(0),
                                      _p(_req(store_off, "store_off", torch.int64)), ctypes.c_double(float(resolution)), c_i64(int(n_point_min)),
                                      _p(h.key), _p(h.order), _p(h.dmin), _p(h.key2), _p(h.order2), _p(h.counts), _p(ws), c_size(ws.numel()),
                                      _stream()), "mcr_scene_fill_begin")
    return h


def scene_fill_gather(g, h, store_pts, store_fts, n_store, F):
    """New store rows = rows g of [old store | admitted candidates of the pending fill h in cell order] -> (pts [n,3], features [n,F] | None)."""
    g = _req(g, "g", torch.int64)
    n, dev = g.numel(), g.device
    new_pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    new_fts = torch.empty((n, F), dtype=torch.float32, device=dev) if F > 0 else None
    with torch.cuda.device(dev):
        check(lib().mcr_scene_fill_gather(_p(g), c_i64(n), _p(store_pts) if n_store else c_vp(0),
                                          _p(store_fts) if (n_store and store_fts is not None) else c_vp(0), c_i64(n_store), c_int(F), _p(h.pts),
                                          _p(h.features) if h.features is not None else c_vp(0), _p(h.order), _p(h.order2), _p(new_pts),
                                          _p(new_fts) if new_fts is not None else c_vp(0), _stream()), "mcr_scene_fill_gather")
    return new_pts, new_fts


def scene_fill_gather_perm(pm_tab, n_pm, n_cells, n_new, h, store_pts, store_fts, n_store, F):
    """As scene_fill_gather with the row map evaluated on the device: pm_tab = ONE uploaded int64 buffer holding the five (n_cells + 1)
    tables of mcr_scene_fill_gather_perm followed (as raw bytes) by the n_pm int32 permutation entries."""
    dev = pm_tab.device
    new_pts = torch.empty((n_new, 3), dtype=torch.float32, device=dev)
    new_fts = torch.empty((n_new, F), dtype=torch.float32, device=dev) if F > 0 else None
    base = pm_tab.data_ptr()
    with torch.cuda.device(dev):
        check(lib().mcr_scene_fill_gather_perm(c_vp(base + 40 * (n_cells + 1)), c_vp(base), c_int(n_cells), c_i64(n_new),
                                               _p(store_pts) if n_store else c_vp(0),
                                               _p(store_fts) if (n_store and store_fts is not None) else c_vp(0), c_i64(n_store), c_int(F),
                                               _p(h.pts), _p(h.features) if h.features is not None else c_vp(0), _p(h.order), _p(h.order2),
                                               _p(new_pts), _p(new_fts) if new_fts is not None else c_vp(0), _stream()),
              "mcr_scene_fill_gather_perm")
    return new_pts, new_fts


class FieldSelection:
    """What mcr_field_select left on the device; `counts` (int64 [3 nk + 9] = visit | sel_counts | sel_off | oof_counts | oof_off)."""
    __slots__ = ("P", "nk", "stored_cell", "rows_order", "oof_order", "counts")


def field_select(proxy_points, supervision_occ, out_of_field, proxy_proba, store_fts, n_store, store_off, grid_consts, grid, use_mask,
                 pending=None):
    """Selection + grouping of the occupancy-field pass (mcr_field_select); proxy_proba is updated in place (:1431)."""
    pp = _req(proxy_points, "proxy_points")
    P, dev = pp.shape[0], pp.device
    nk = grid[0] * grid[1] * grid[2]
    for name, t in (("proxy_supervision_occ", supervision_occ), ("out_of_field", out_of_field), ("proxy_proba", proxy_proba)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == P):
            raise ValueError(f"{name} must be a contiguous fp32 device tensor with one entry per proxy point")
    F = store_fts.shape[1] if (store_fts is not None and store_fts.dim() == 2) else 1
    if pending is not None and (pending.features is None or pending.features.shape[1] != F):
        raise ValueError("field_select: the pending fill carries no features (the proxy indices)")
    s = FieldSelection()
    s.P, s.nk = P, nk
    ib = torch.empty(5 * P, dtype=torch.int32, device=dev)
    s.stored_cell, key_sel, key_oof, s.rows_order, s.oof_order = (ib[k * P:(k + 1) * P] for k in range(5))
    s.counts = torch.empty(3 * nk + 9, dtype=torch.int64, device=dev)
    L_ = lib()
    ws = _entry_workspace(dev, L_.mcr_field_select_workspace_bytes, c_i64(P), c_int(nk))
    pe = pending
    with torch.cuda.device(dev):
        check(L_.mcr_field_select(_p(pp), c_i64(P), _p(supervision_occ), _p(out_of_field), _p(proxy_proba),
                                  _p(store_fts) if n_store else c_vp(0), c_int(F), c_i64(n_store), _p(_req(store_off, "store_off", torch.int64)),
                                  _p(pe.features) if pe is not None else c_vp(0), _p(pe.order) if pe is not None else c_vp(0),
                                  _p(pe.order2) if pe is not None else c_vp(0), _p(pe.key2) if pe is not None else c_vp(0),
                                  c_vp(pe.counts.data_ptr() + 8 * (3 * nk + 4)) if pe is not None else c_vp(0), c_i64(pe.N if pe is not None else 0),
                                  _p(_req(grid_consts, "grid_consts")), c_int(grid[0]), c_int(grid[1]), c_int(grid[2]), c_int(int(bool(use_mask))),
                                  _p(s.stored_cell), _p(key_sel), _p(key_oof), _p(s.rows_order), _p(s.oof_order), _p(s.counts), _p(ws),
                                  c_size(ws.numel()), _stream()), "mcr_field_select")
    return s


# The uploaded table of the occupancy passes: J job rows (4 int64) | n_seg surface-segment rows (4 int64) | J transforms (20 fp32) | the
# bin permutation (int32) | whatever the caller appends
FIELD_JOB_ROW_BYTES, FIELD_SEGMENT_ROW_BYTES, FIELD_TRANSFORM_ROW_BYTES = 32, 32, 80


def field_table_offsets(J, n_seg):
    """Byte offsets of (segment table, transform table, bin permutation) in the uploaded table of J jobs and n_seg segments."""
    o_seg = FIELD_JOB_ROW_BYTES * J
    o_xf = o_seg + FIELD_SEGMENT_ROW_BYTES * n_seg
    return o_seg, o_xf, o_xf + FIELD_TRANSFORM_ROW_BYTES * J


def field_build(tables, J, n_seg, sel, proxy_points, S_all, view_states, bin_perm, vh_matrix_t, T, tot, X_world, vh):
    """The jobs of the occupancy-field pass (mcr_field_build).  tables: ONE uploaded fp64-free buffer = int64 [J*4 + n_seg*4] followed
    (as raw bytes) by fp32 [J*20] (field_table_offsets); X_world [>=T,3] and vh [>=T,64] are written in their first T rows.
    -> (rows int32 [T], row_job int32 [T], X_q [T,3], pc_all [tot,3])."""
    dev = proxy_points.device
    ib = torch.empty(2 * T, dtype=torch.int32, device=dev)
    rows, row_job = ib[:T], ib[T:]
    fb = torch.empty(3 * (T + tot), dtype=torch.float32, device=dev)
    X_q, pc_all = fb[:3 * T].view(T, 3), fb[3 * T:].view(tot, 3)
    base = tables.data_ptr()
    o_seg, o_xf, _ = field_table_offsets(J, n_seg)
    n_bins = view_states.shape[1]
    with torch.cuda.device(dev):
        check(lib().mcr_field_build(c_vp(base), c_int(J), c_vp(base + o_seg), c_int(n_seg), c_vp(base + o_xf), _p(sel.rows_order),
                                    _p(proxy_points), _p(S_all), _p(view_states), c_int(n_bins), _p(bin_perm) if bin_perm is not None else c_vp(0),
                                    _p(vh_matrix_t), c_i64(T),
                                    c_i64(tot), _p(rows), _p(row_job), _p(X_world), _p(X_q), _p(vh), _p(pc_all), _stream()), "mcr_field_build")
    return rows, row_job, X_q, pc_all


def view_harmonics_rows(view_states, rows, bin_perm, vh_matrix_t, out=None):
    """vh [T,64] of rows `rows` (int32 device, None = all) of a view-state table: bins permuted by bin_perm (int32 device, None = identity),
    then the [n_bins, 64] product (mcr_view_harmonics_rows)."""
    vs = _req(view_states, "view_states")
    T = rows.numel() if rows is not None else vs.shape[0]
    if out is None:
        out = torch.empty((T, 64), dtype=torch.float32, device=vs.device)
    if T == 0:
        return out
    with torch.cuda.device(vs.device):
        check(lib().mcr_view_harmonics_rows(_p(vs), c_int(vs.shape[1]), _p(rows) if rows is not None else c_vp(0),
                                            _p(bin_perm) if bin_perm is not None else c_vp(0), _p(_req(vh_matrix_t, "vh_matrix_t")), c_i64(T),
                                            _p(out), _stream()), "mcr_view_harmonics_rows")
    return out


def field_finish(rows, occ, T, proxy_proba, sel, n_oof, proxy_points, X_tail, occ_tail):
    with torch.cuda.device(proxy_points.device):
        check(lib().mcr_field_finish(_p(rows) if T else c_vp(0), _p(occ) if T else c_vp(0), c_i64(T), _p(proxy_proba), _p(sel.oof_order),
                                     c_i64(n_oof), _p(proxy_points), _p(X_tail) if n_oof else c_vp(0), _p(occ_tail) if n_oof else c_vp(0),
                                     _stream()), "mcr_field_finish")


class SupervisionSelection:
    """What mcr_supervision_select left on the device; `counts` (int64 [3 nk + 5] = englobing | sel_counts | sel_off | n_pred), `pos`
    (int32 [P]: row of every sampled point in the pass's result, -1 elsewhere), `rows_order` as FieldSelection's."""
    __slots__ = ("P", "nk", "rows_order", "counts", "pos")


def supervision_select(prediction_mask, proxy_points, grid_consts, grid, store_fts, n_store, store_off):
    """Selection of the supervision pass (mcr_supervision_select): prediction_mask [P] (bool / uint8, device)."""
    pp = _req(proxy_points, "proxy_points")
    P, dev = pp.shape[0], pp.device
    nk = grid[0] * grid[1] * grid[2]
    if not (isinstance(prediction_mask, torch.Tensor) and prediction_mask.is_cuda and prediction_mask.numel() == P
            and prediction_mask.dtype in (torch.bool, torch.uint8)):
        raise ValueError("prediction_mask must be a bool / uint8 device tensor with one entry per proxy point")
    m8 = prediction_mask.reshape(-1).contiguous().view(torch.uint8)
    F = store_fts.shape[1] if (store_fts is not None and store_fts.dim() == 2) else 1
    if n_store and (store_fts is None or store_fts.shape[0] < n_store):
        raise ValueError("supervision_select: the store's features (the proxy indices) are missing")
    s = SupervisionSelection()
    s.P, s.nk = P, nk
    ib = torch.empty(P + max(n_store, 1), dtype=torch.int32, device=dev)
    s.pos, s.rows_order = ib[:P], ib[P:]
    s.counts = torch.empty(3 * nk + 5, dtype=torch.int64, device=dev)
    L_ = lib()
    ws = _entry_workspace(dev, L_.mcr_supervision_select_workspace_bytes, c_i64(P), c_int(nk))
    with torch.cuda.device(dev):
        check(L_.mcr_supervision_select(_p(m8), _p(pp), c_i64(P), _p(_req(grid_consts, "grid_consts")), c_int(grid[0]), c_int(grid[1]),
                                        c_int(grid[2]), _p(_req(store_fts, "store_fts")) if n_store else c_vp(0), c_int(F), c_i64(n_store),
                                        _p(_req(store_off, "store_off", torch.int64)), _p(s.rows_order), c_i64(s.rows_order.numel()),
                                        _p(s.counts), _p(s.pos), _p(ws), c_size(ws.numel()), _stream()), "mcr_supervision_select")
    return s


def supervision_scatter(rows, occ, job_offsets, J, pos, n_out):
    """out [n_out,1]: out[pos[rows[t]]] += occ[t] from zeros over the rows of the first J jobs, in job order (mcr_supervision_scatter).
    rows int32 [>= job_offsets[J]], occ fp32 (same rows), job_offsets int64 device [>= J+1], pos int32 [P]."""
    pos = _req(pos, "pos", torch.int32)
    out = torch.zeros((n_out, 1), dtype=torch.float32, device=pos.device)
    if J == 0 or n_out == 0:
        return out
    with torch.cuda.device(pos.device):
        check(lib().mcr_supervision_scatter(_p(_req(rows, "rows", torch.int32)), _p(_req(occ, "occ")), _p(_req(job_offsets, "job_offsets", torch.int64)),
                                            c_int(J), _p(pos), c_i64(pos.numel()), _p(out), c_i64(n_out), _stream()), "mcr_supervision_scatter")
    return out


def supervision_scatter_backward(rows, pos, d_out, T_scatter, T):
    """d_occ [T,1] = d_out[pos[rows[t]]] for t < T_scatter, 0 behind (mcr_supervision_scatter_backward)."""
    pos = _req(pos, "pos", torch.int32)
    d_occ = torch.zeros((T, 1), dtype=torch.float32, device=pos.device)
    if T == 0 or T_scatter == 0 or d_out.numel() == 0:
        return d_occ
    with torch.cuda.device(pos.device):
        check(lib().mcr_supervision_scatter_backward(_p(_req(rows, "rows", torch.int32)), _p(pos), c_i64(pos.numel()), _p(_req(d_out, "d_out")),
                                                     c_i64(d_out.numel()), c_i64(T_scatter), c_i64(T), _p(d_occ), _stream()),
              "mcr_supervision_scatter_backward")
    return d_occ


def camera_boxes(sampled, n_unique, M_view, cam_world, inv_diag):
    """sampled [K,S,4], n_unique int32 [K], M_view [K,4,4], cam_world [K,3] -> (centre [K,3] of each camera's prediction box in view space,
    camera centres [K,3] in the normalised prediction space)   (mcr_camera_boxes)."""
    sampled = _req(sampled, "sampled")
    K, S = sampled.shape[0], sampled.shape[1]
    out = torch.empty((2, K, 3), dtype=torch.float32, device=sampled.device)
    with torch.cuda.device(sampled.device):
        check(lib().mcr_camera_boxes(_p(sampled), _p(_req(n_unique, "n_unique", torch.int32)), c_i64(K), c_int(S), _p(_req(M_view, "M_view")),
                                     _p(_req(cam_world, "cam_world")), c_f32(float(inv_diag)), _p(out[0]), _p(out[1]), _stream()),
              "mcr_camera_boxes")
    return out[0], out[1]


def macarons_gain_indexed(vis_unique, world_unique, inverse, n_unique, cam_world, volume, distance_th, smooth=False):
    """gains [K] from the per-UNIQUE-point visibility gains vis_unique [K,S] and the inverse map of the Monte-Carlo samples
    (mcr_macarons_gain_indexed)."""
    vis_unique, world_unique = _req(vis_unique, "vis_unique"), _req(world_unique, "world_unique")
    K, S = vis_unique.shape
    gains = torch.empty(K, dtype=torch.float32, device=vis_unique.device)
    with torch.cuda.device(vis_unique.device):
        check(lib().mcr_macarons_gain_indexed(_p(vis_unique), _p(world_unique), _p(_req(inverse, "inverse", torch.int64)),
                                              _p(_req(n_unique, "n_unique", torch.int32)), _p(_req(cam_world, "cam_world")),
                                              _p(_req(volume, "volume")), c_f32(float(distance_th)), c_int(int(bool(smooth))), c_i64(K), c_int(S),
                                              _p(gains), _stream()), "mcr_macarons_gain_indexed")
    return gains


def macarons_gain_backward(grad_gains, vis, world, inverse, n_unique, cam_world, volume, distance_th, smooth=False, need_volume=False):
    """(d_vis [K,S], d_volume [K] or None): gradients of macarons_gain_indexed for grad_gains [K] with respect to the per-unique-point
    gains vis [K,S] and, with need_volume, the volumes (mcr_macarons_gain_backward).  world [K,S,>=3].  inverse None and n_unique None:
    the identity map, every camera non-empty -- the backward of macarons_gain_ (vis = its input before the in-place scaling)."""
    grad_gains, vis, world = _req(grad_gains, "grad_gains"), _req(vis, "vis"), _req(world, "world")
    if (inverse is None) != (n_unique is None):
        raise ValueError("inverse and n_unique go together (both None: the identity form)")
    K, S = vis.shape
    if grad_gains.shape != (K,):
        raise ValueError(f"grad_gains must be [K] = {(K,)}, got {tuple(grad_gains.shape)}")
    if world.dim() != 3 or world.shape[:2] != (K, S) or world.shape[2] < 3:
        raise ValueError(f"world must be [K,S,>=3] with [K,S] = {(K, S)}, got {tuple(world.shape)}")
    if inverse is not None and tuple(inverse.shape) != (K, S):
        raise ValueError(f"inverse must be [K,S] = {(K, S)}, got {tuple(inverse.shape)}")
    if inverse is not None:
        inverse, n_unique = _req(inverse, "inverse", torch.int64), _req(n_unique, "n_unique", torch.int32)
        if n_unique.numel() != K:
            raise ValueError(f"n_unique must be [K] = {(K,)}, got {tuple(n_unique.shape)}")
    cam_world, volume = _req(cam_world, "cam_world"), _req(volume, "volume")
    if cam_world.numel() != 3 * K or volume.numel() != K:
        raise ValueError(f"cam_world must be [K,3] and volume [K] with K = {K}, got {tuple(cam_world.shape)} and {tuple(volume.shape)}")
    d_vis = torch.empty((K, S), dtype=torch.float32, device=vis.device)
    d_volume = torch.empty(K, dtype=torch.float32, device=vis.device) if need_volume else None
    with torch.cuda.device(vis.device):
        check(lib().mcr_macarons_gain_backward(_p(grad_gains), _p(vis), _p(world), c_int(world.shape[2]),
                                               _p(inverse) if inverse is not None else c_vp(0),
                                               _p(n_unique) if n_unique is not None else c_vp(0),
                                               _p(cam_world), _p(volume), c_f32(float(distance_th)),
                                               c_int(int(bool(smooth))), c_i64(K), c_int(S), _p(d_vis),
                                               _p(d_volume) if need_volume else c_vp(0), _stream()), "mcr_macarons_gain_backward")
    return d_vis, d_volume


_PHILOX_MAPPING = 1          # rocRAND's (0, 1] map (what torch.rand uses on ROCm); tests/test_glue_gpu.py pins it against torch.rand


def uniform_rows(K, S, device, generator=None):
    """[K, S] uniforms = what K consecutive torch.rand(S, 1, device=device) calls return (upstream's per-camera sampling draws,
    scone_utils.py:1052), from ONE launch; the device generator advances exactly as those K calls would advance it."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = generator if generator is not None else torch.cuda.default_generators[idx]
    if S > 65536:                                    # beyond one element per thread torch's kernel changes its indexing: the literal draws
        return torch.cat([torch.rand(S, 1, device=device, generator=generator) for _ in range(K)], 1).t().contiguous()
    seed, off = gen.initial_seed(), gen.get_offset()
    out = torch.empty((K, S), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(lib().mcr_philox_uniform_rows(ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(off), c_i64(K), c_int(S),
                                            c_int(_PHILOX_MAPPING), _p(out), _stream()), "mcr_philox_uniform_rows")
    gen.set_offset(off + 4 * K)
    return out


# ---- depth module: the plane sweep ---------------------------------------------------------------------------------------------
COST_VOLUME_FOV_SCALE = 1.0 / float(np.tan(np.deg2rad(60.0) / 2))    # FoVPerspectiveCameras' default fov, which upstream never overrides


def _cost_volume_args(x, x_alpha, cams, depth_bins):
    x, x_alpha, cams, depth_bins = _req(x, "x"), _req(x_alpha, "x_alpha"), _req(cams, "cams"), _req(depth_bins, "depth_bins")
    if x.dim() != 4 or x_alpha.dim() != 5:
        raise ValueError(f"x must be [B,C,Hf,Wf] and x_alpha [B,A,C,Hf,Wf]; got {tuple(x.shape)}, {tuple(x_alpha.shape)}")
    B, C, Hf, Wf = x.shape
    A, D = x_alpha.shape[1], depth_bins.numel()
    if tuple(x_alpha.shape) != (B, A, C, Hf, Wf):
        raise ValueError(f"x_alpha must be [B,A,C,Hf,Wf] = {(B, A, C, Hf, Wf)}, got {tuple(x_alpha.shape)}")
    if tuple(cams.shape) != (B, 1 + A, 12):
        raise ValueError(f"cams must be [B,1+A,12] = {(B, 1 + A, 12)}, got {tuple(cams.shape)}")
    return x, x_alpha, cams, depth_bins, B, A, C, Hf, Wf, D


def cost_volume(x, x_alpha, cams, depth_bins, H, W, fov_scale=COST_VOLUME_FOV_SCALE, out=None):
    """cost volume [B,D,Hf,Wf] of CostVolumeBuilder.forward (ManyDepth.py:207-297) in one entry (mcr_cost_volume): x [B,64,Hf,Wf] target
    features, x_alpha [B,A,64,Hf,Wf] source features, cams [B,1+A,12] (row 0 the target, then the sources; R row-major then T, PyTorch3D's
    row-vector convention), depth_bins [D], H x W the image size whose pixel grid is unprojected.  out: None, or a [B,D,Hf,Wf] float32
    view whose batches may be strided -- channels C.. of a [B,C+D,Hf,Wf] buffer, where upstream's torch.cat puts the volume."""
    x, x_alpha, cams, depth_bins, B, A, C, Hf, Wf, D = _cost_volume_args(x, x_alpha, cams, depth_bins)
    if out is None:
        out = torch.empty((B, D, Hf, Wf), dtype=torch.float32, device=x.device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or out.dtype != torch.float32:
            raise MacaronsHipError("out must be a float32 tensor on x's HIP device")
        if tuple(out.shape) != (B, D, Hf, Wf) or (B * D * Hf * Wf and out[0].stride() != (Hf * Wf, Wf, 1)):
            raise ValueError(f"out must be [B,D,Hf,Wf] = {(B, D, Hf, Wf)} with contiguous batches, got {tuple(out.shape)} strides {out.stride()}")
    L = lib()
    ws = _entry_workspace(x.device, L.mcr_cost_volume_workspace_bytes, c_i64(B), c_i64(A), c_i64(C), c_i64(Hf), c_i64(Wf))
    with torch.cuda.device(x.device):
        check(L.mcr_cost_volume(_p(x), _p(x_alpha), _p(cams), _p(depth_bins), _p(out), c_i64(out.stride(0) if B > 1 else D * Hf * Wf),
                                c_i64(B), c_int(A), c_int(C), c_int(int(H)), c_int(int(W)), c_int(Hf), c_int(Wf), c_int(D),
                                c_f32(float(fov_scale)), _p(ws), c_size(ws.numel()), _stream()), "mcr_cost_volume")
    return out


def cost_volume_backward(x, x_alpha, cams, depth_bins, d_out, H, W, fov_scale=COST_VOLUME_FOV_SCALE, need_x=True, need_x_alpha=True):
    """(d_x [B,64,Hf,Wf] | None, d_x_alpha [B,A,64,Hf,Wf] | None): the gradients of cost_volume's x and x_alpha for the upstream gradient
    d_out [B,D,Hf,Wf], in one entry (mcr_cost_volume_backward, csrc/cost_volume_bwd.hip); the cameras and the bins are constants.  d_out's
    batches may be strided -- channels C.. of the gradient of a [B,C+D,Hf,Wf] buffer.  A gradient that is not needed is not computed
    (the x_alpha half is the expensive one).  No floating-point atomics: two calls give the same bits.  A d_out that is not finite gives
    gradients of NaN."""
    x, x_alpha, cams, depth_bins, B, A, C, Hf, Wf, D = _cost_volume_args(x, x_alpha, cams, depth_bins)
    if not isinstance(d_out, torch.Tensor) or not d_out.is_cuda or d_out.device != x.device or d_out.dtype != torch.float32:
        raise MacaronsHipError("d_out must be a float32 tensor on x's HIP device")
    if tuple(d_out.shape) != (B, D, Hf, Wf):
        raise ValueError(f"d_out must be [B,D,Hf,Wf] = {(B, D, Hf, Wf)}, got {tuple(d_out.shape)}")
    if not need_x and not need_x_alpha:
        raise ValueError("cost_volume_backward: nothing to do, neither gradient is needed")
    if B * D * Hf * Wf and (d_out[0].stride() != (Hf * Wf, Wf, 1) or (B > 1 and d_out.stride(0) < D * Hf * Wf)):
        d_out = d_out.contiguous()
    d_x = torch.empty_like(x) if need_x else None
    d_xa = torch.empty_like(x_alpha) if need_x_alpha else None
    L = lib()
    ws = _entry_workspace(x.device, L.mcr_cost_volume_backward_workspace_bytes, c_i64(B), c_i64(A), c_i64(C), c_i64(Hf), c_i64(Wf), c_i64(D))
    with torch.cuda.device(x.device):
        check(L.mcr_cost_volume_backward(_p(x), _p(x_alpha), _p(cams), _p(depth_bins), _p(d_out),
                                         c_i64(d_out.stride(0) if B > 1 else D * Hf * Wf), _p(d_x) if need_x else None,
                                         _p(d_xa) if need_x_alpha else None, c_i64(B), c_int(A), c_int(C), c_int(int(H)), c_int(int(W)),
                                         c_int(Hf), c_int(Wf), c_int(D), c_f32(float(fov_scale)), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_cost_volume_backward")
    return d_x, d_xa


# ---- depth module: the photometric reconstruction loss ------------------------------------------------------------------------------
RECONSTRUCTION_PADDING_MODES = {"zeros": 0, "border": 1}


def _reconstruction_args(images, alpha_images, mask, cams, depth, padding_mode):
    images, alpha_images, cams, depth = _req(images, "images"), _req(alpha_images, "alpha_images"), _req(cams, "cams"), _req(depth, "depth")
    if images.dim() != 4 or images.shape[-1] != 3 or alpha_images.dim() != 5 or depth.dim() != 4:
        raise ValueError(f"images must be [B,H,W,3], alpha_images [B,A,H,W,3] and depth [S,B,H,W]; got {tuple(images.shape)}, "
                         f"{tuple(alpha_images.shape)}, {tuple(depth.shape)}")
    B, H, W, _ = images.shape
    A, S = alpha_images.shape[1], depth.shape[0]
    if tuple(alpha_images.shape) != (B, A, H, W, 3):
        raise ValueError(f"alpha_images must be [B,A,H,W,3] = {(B, A, H, W, 3)}, got {tuple(alpha_images.shape)}")
    if tuple(depth.shape) != (S, B, H, W):
        raise ValueError(f"depth must be [S,B,H,W] = {(S, B, H, W)}, got {tuple(depth.shape)}")
    if tuple(cams.shape) != (B, 1 + A, 12):
        raise ValueError(f"cams must be [B,1+A,12] = {(B, 1 + A, 12)}, got {tuple(cams.shape)}")
    if mask is not None:
        mask = _req(mask, "mask", torch.bool)
        if tuple(mask.shape) != (B, H, W):
            raise ValueError(f"mask must be [B,H,W] = {(B, H, W)}, got {tuple(mask.shape)}")
    if padding_mode not in RECONSTRUCTION_PADDING_MODES:
        raise ValueError(f"padding_mode must be one of {sorted(RECONSTRUCTION_PADDING_MODES)} here, got {padding_mode!r} "
                         "(networks.ManyDepth.reconstruction_loss_composite takes 'reflection')")
    return images, alpha_images, mask, cams, depth, (S, B, A, H, W), RECONSTRUCTION_PADDING_MODES[padding_mode]


def reconstruction_loss(images, alpha_images, mask, cams, depth, zfar, ssim_factor, padding_mode="border", fov_scale=COST_VOLUME_FOV_SCALE,
                        return_map=False):
    """loss [S] of upstream's reconstruction_loss_fn (macarons_utils.py:1120-1185) for S depth maps in one entry (mcr_reconstruction_loss):
    images [B,H,W,3], alpha_images [B,A,H,W,3], mask [B,H,W] bool or None (None = params.use_depth_mask False), cams [B,1+A,12]
    (networks.ManyDepth.pack_cameras), depth [S,B,H,W]; padding_mode 'zeros' or 'border'.  return_map: (loss, loss_map [S,B,H,W] the
    selected per-pixel loss, argmin [S,B,H,W] uint8 its source)."""
    images, alpha_images, mask, cams, depth, (S, B, A, H, W), mode = _reconstruction_args(images, alpha_images, mask, cams, depth, padding_mode)
    loss = torch.empty((S,), dtype=torch.float32, device=images.device)
    lmap = torch.empty((S, B, H, W), dtype=torch.float32, device=images.device) if return_map else None
    amin = torch.empty((S, B, H, W), dtype=torch.uint8, device=images.device) if return_map else None
    L = lib()
    ws = _entry_workspace(images.device, L.mcr_reconstruction_loss_workspace_bytes, c_i64(S), c_i64(B), c_i64(A), c_i64(H), c_i64(W))
    with torch.cuda.device(images.device):
        check(L.mcr_reconstruction_loss(_p(images), _p(alpha_images), _p(mask) if mask is not None else None, _p(cams), _p(depth), _p(loss),
                                        _p(lmap) if return_map else None, _p(amin) if return_map else None, c_i64(S), c_i64(B), c_int(A),
                                        c_int(H), c_int(W), c_f32(float(fov_scale)), c_f32(float(zfar)), c_f32(float(ssim_factor)),
                                        c_int(mode), _p(ws), c_size(ws.numel()), _stream()), "mcr_reconstruction_loss")
    return (loss, lmap, amin) if return_map else loss


def reconstruction_loss_backward(images, alpha_images, mask, cams, depth, d_loss, zfar, ssim_factor, padding_mode="border",
                                 fov_scale=COST_VOLUME_FOV_SCALE):
    """d_depth [S,B,H,W]: the gradient of sum_s d_loss[s] * reconstruction_loss(...)[s] for depth, in one entry
    (mcr_reconstruction_loss_backward); the images, the cameras and the mask are constants.  No atomics: two calls give the same bits."""
    images, alpha_images, mask, cams, depth, (S, B, A, H, W), mode = _reconstruction_args(images, alpha_images, mask, cams, depth, padding_mode)
    d_loss = _req(d_loss, "d_loss")
    if tuple(d_loss.shape) != (S,):
        raise ValueError(f"d_loss must be [S] = {(S,)}, got {tuple(d_loss.shape)}")
    d_depth = torch.empty((S, B, H, W), dtype=torch.float32, device=images.device)
    L = lib()
    ws = _entry_workspace(images.device, L.mcr_reconstruction_loss_backward_workspace_bytes, c_i64(S), c_i64(B), c_i64(A), c_i64(H), c_i64(W))
    with torch.cuda.device(images.device):
        check(L.mcr_reconstruction_loss_backward(_p(images), _p(alpha_images), _p(mask) if mask is not None else None, _p(cams), _p(depth),
                                                 _p(d_loss), _p(d_depth), c_i64(S), c_i64(B), c_int(A), c_int(H), c_int(W),
                                                 c_f32(float(fov_scale)), c_f32(float(zfar)), c_f32(float(ssim_factor)), c_int(mode), _p(ws),
                                                 c_size(ws.numel()), _stream()), "mcr_reconstruction_loss_backward")
    return d_depth


# ---- depth module: disparity scales, regularity values and the error mask -------------------------------------------------------------
DISPARITY_SCALE_RATIOS = (1, 2, 4, 8, 16)
DISPARITY_MAX_SCALES = 8


def _disparity_args(disps, images, mask):
    """The shapes first (ValueError, on any device), then the operands themselves (HIP, float32, contiguous)."""
    if isinstance(disps, torch.Tensor) or not len(disps):
        raise ValueError("disps must be a non-empty sequence of [B,1,H_s,W_s] or [B,H_s,W_s] tensors, one per scale")
    if not 1 <= len(disps) <= DISPARITY_MAX_SCALES:
        raise ValueError(f"between 1 and {DISPARITY_MAX_SCALES} scales are supported, got {len(disps)}")
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"images must be [B,H,W,3], got {tuple(getattr(images, 'shape', ()))}")
    B, H, W, _ = images.shape
    if H < 2 or W < 2:
        raise ValueError(f"the image is {H} x {W}, H and W must be at least 2")
    maps, sizes = [], []
    for s, d in enumerate(disps):
        if not isinstance(d, torch.Tensor):
            raise TypeError(f"disps[{s}] must be a torch.Tensor")
        if d.dim() == 4 and d.shape[1] == 1:
            d = d[:, 0]
        if d.dim() != 3 or d.shape[0] != B or d.shape[1] < 1 or d.shape[2] < 1:
            raise ValueError(f"disps[{s}] must be [B,1,H_s,W_s] or [B,H_s,W_s] with B = {B}, got {tuple(disps[s].shape)}")
        Hs, Ws = int(d.shape[1]), int(d.shape[2])
        r = H // Hs
        if r not in DISPARITY_SCALE_RATIOS or Hs * r != H or Ws * r != W:
            raise ValueError(f"disps[{s}] is {Hs} x {Ws} for an image of {H} x {W}: the ratio must be one of {DISPARITY_SCALE_RATIOS}, the "
                             "same on both axes (networks.ManyDepth.disparity_scales_composite takes other sizes)")
        maps.append(d), sizes.append((Hs, Ws))
    if mask is not None and (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, H, W)):
        raise ValueError(f"mask must be [B,H,W] = {(B, H, W)}, got {tuple(getattr(mask, 'shape', ()))}")
    images = _req(images, "images")
    maps = [_req(d, f"disps[{s}]") for s, d in enumerate(maps)]
    if mask is not None:
        mask = _req(mask, "mask", torch.bool)
    S = len(maps)
    ptrs = (ctypes.c_void_p * S)(*[d.data_ptr() for d in maps])
    hs, wss = (ctypes.c_int * S)(*[h for h, _ in sizes]), (ctypes.c_int * S)(*[w for _, w in sizes])
    return maps, images, mask, (S, B, H, W), (ptrs, hs, wss)


def disparity_scales(disps, images, mask, znear, zfar, return_tab=False):
    """(depth [S,B,H,W], reg [S], error_mask [B,H,W] bool) of S disparity maps in one entry (mcr_disparity_scales): what upstream's
    apply_depth_model does between the depth network and its losses (macarons_utils.py:959-1031).  disps: a sequence of [B,1,H_s,W_s] or
    [B,H_s,W_s] float32 maps, each 1, 2, 4, 8 or 16 times smaller than the images on both axes (they are not concatenated: the kernels
    take the S pointers); images [B,H,W,3]; mask [B,H,W] bool or None.  depth is the layout ops.reconstruction_loss reads; reg[s] is the
    raw regularity value of scale s (the scale weights and params.regularity_factor stay with the caller); error_mask is upstream's
    `error_tab < mean + std` of scale 0.  return_tab: also tab [B,H,W] and thr [B]."""
    maps, images, mask, (S, B, H, W), (ptrs, hs, wss) = _disparity_args(disps, images, mask)
    dev = images.device
    depth = torch.empty((S, B, H, W), dtype=torch.float32, device=dev)
    reg = torch.empty((S,), dtype=torch.float32, device=dev)
    em = torch.empty((B, H, W), dtype=torch.bool, device=dev)
    tab = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_tab else None
    thr = torch.empty((B,), dtype=torch.float32, device=dev) if return_tab else None
    L = lib()
    ws = _entry_workspace(dev, L.mcr_disparity_scales_workspace_bytes, c_i64(S), c_i64(B), c_i64(H), c_i64(W))
    with torch.cuda.device(dev):
        check(L.mcr_disparity_scales(ptrs, hs, wss, _p(images), _p(mask) if mask is not None else None, _p(depth), _p(reg), _p(em),
                                     _p(tab) if return_tab else None, _p(thr) if return_tab else None, c_int(S), c_i64(B), c_int(H), c_int(W),
                                     c_f32(float(znear)), c_f32(float(zfar)), _p(ws), c_size(ws.numel()), _stream()), "mcr_disparity_scales")
    return (depth, reg, em, tab, thr) if return_tab else (depth, reg, em)


def disparity_scales_backward(disps, images, mask, znear, zfar, d_depth, d_reg):
    """The S gradients [B,H_s,W_s] of sum(d_depth * depth) + sum(d_reg * reg) of disparity_scales for the disparities, each at its own
    resolution, in one entry (mcr_disparity_scales_backward).  d_depth [S,B,H,W] or None, d_reg [S] or None: a half that is None is not
    computed, both None is refused.  No atomics: two calls give the same bits."""
    if d_depth is None and d_reg is None:
        raise ValueError("disparity_scales_backward: nothing to do, d_depth and d_reg are both None")
    maps, images, mask, (S, B, H, W), (ptrs, hs, wss) = _disparity_args(disps, images, mask)
    if d_depth is not None:
        if not isinstance(d_depth, torch.Tensor) or tuple(d_depth.shape) != (S, B, H, W):
            raise ValueError(f"d_depth must be [S,B,H,W] = {(S, B, H, W)}, got {tuple(getattr(d_depth, 'shape', ()))}")
        d_depth = _req(d_depth, "d_depth")
    if d_reg is not None:
        if not isinstance(d_reg, torch.Tensor) or tuple(d_reg.shape) != (S,):
            raise ValueError(f"d_reg must be [S] = {(S,)}, got {tuple(getattr(d_reg, 'shape', ()))}")
        d_reg = _req(d_reg, "d_reg")
    grads = [torch.empty_like(d) for d in maps]
    gptrs = (ctypes.c_void_p * S)(*[g.data_ptr() for g in grads])
    L = lib()
    ws = _entry_workspace(images.device, L.mcr_disparity_scales_backward_workspace_bytes, c_i64(S), c_i64(B), c_i64(H), c_i64(W))
    with torch.cuda.device(images.device):
        check(L.mcr_disparity_scales_backward(ptrs, hs, wss, _p(images), _p(mask) if mask is not None else None,
                                              _p(d_depth) if d_depth is not None else None, _p(d_reg) if d_reg is not None else None, gptrs,
                                              c_int(S), c_i64(B), c_int(H), c_int(W), c_f32(float(znear)), c_f32(float(zfar)), _p(ws),
                                              c_size(ws.numel()), _stream()), "mcr_disparity_scales_backward")
    return grads


# ---- depth module: the disparity heads (reflect 3x3 convolution to one channel + sigmoid) -------------------------------------------------
DISPARITY_HEAD_MAX_CHANNELS = 512


def _disparity_head_args(x, weight, bias=None, maps=()):
    """The shapes first (ValueError, on any device), then the operands themselves (HIP, float32, contiguous).  weight: upstream's
    conv.weight [1,C,3,3] or [C,3,3]; bias [1] (None: not needed, the backward); maps: (name, [B,1,Hs,Ws] or [B,Hs,Ws]) pairs."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"x must be [B,C,Hs,Ws], got {tuple(getattr(x, 'shape', ()))}")
    B, C, Hs, Ws = (int(v) for v in x.shape)
    if B < 1 or not 1 <= C <= DISPARITY_HEAD_MAX_CHANNELS:
        raise ValueError(f"x is {tuple(x.shape)}: B must be at least 1 and C between 1 and {DISPARITY_HEAD_MAX_CHANNELS}")
    if Hs < 2 or Ws < 2:
        raise ValueError(f"the map is {Hs} x {Ws}, Hs and Ws must be at least 2 (the reflection padding)")
    if B * C * Hs * Ws > 2 ** 31 - 1:
        raise ValueError(f"x is {tuple(x.shape)}: its size overflows a 32-bit index")
    if not isinstance(weight, torch.Tensor) or tuple(weight.shape) not in ((1, C, 3, 3), (C, 3, 3)):
        raise ValueError(f"weight must be [1,C,3,3] or [C,3,3] with C = {C}, got {tuple(getattr(weight, 'shape', ()))}")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.numel() != 1):
        raise ValueError(f"bias must hold one value, got {tuple(getattr(bias, 'shape', ()))}")
    for name, m in maps:
        if not isinstance(m, torch.Tensor) or tuple(m.shape) not in ((B, 1, Hs, Ws), (B, Hs, Ws)):
            raise ValueError(f"{name} must be [B,1,Hs,Ws] or [B,Hs,Ws] = {(B, Hs, Ws)}, got {tuple(getattr(m, 'shape', ()))}")
    x, weight = _req(x, "x"), _req(weight, "weight")
    if bias is not None:
        bias = _req(bias, "bias")
    return x, weight, bias, (B, C, Hs, Ws), [_req(m, name) for name, m in maps]


def disparity_head(x, weight, bias, return_z=False):
    """y [B,1,Hs,Ws] = sigmoid(conv3x3(reflection_pad(x), weight) + bias) in one entry (mcr_disparity_head): upstream's DisparityLayer
    (ManyDepth.py:366-384).  x [B,C,Hs,Ws], weight [1,C,3,3] or [C,3,3], bias [1], float32.  return_z: also the pre-activation z
    [B,1,Hs,Ws].  The same bits on every call."""
    x, weight, bias, (B, C, Hs, Ws), _ = _disparity_head_args(x, weight, bias)
    y = torch.empty((B, 1, Hs, Ws), dtype=torch.float32, device=x.device)
    z = torch.empty_like(y) if return_z else None
    with torch.cuda.device(x.device):
        check(lib().mcr_disparity_head(_p(x), _p(weight), _p(bias), _p(y), _p(z) if return_z else None, c_i64(B), c_int(C), c_int(Hs),
                                       c_int(Ws), _stream()), "mcr_disparity_head")
    return (y, z) if return_z else y


def disparity_head_backward(x, weight, y, d_y, need=(True, True, True)):
    """(d_x [B,C,Hs,Ws], d_weight in weight's shape, d_bias [1]) of sum(d_y * y) for y = disparity_head(x, weight, bias), in one entry
    (mcr_disparity_head_backward); y and d_y [B,1,Hs,Ws] or [B,Hs,Ws].  need: which of the three are computed, the others are None
    (d_x alone does not read x); all False is refused.  No atomics: two calls give the same bits."""
    need = tuple(bool(n) for n in need)
    if len(need) != 3 or not any(need):
        raise ValueError("disparity_head_backward: need must name at least one of (d_x, d_weight, d_bias)")
    x, weight, _, (B, C, Hs, Ws), (y, d_y) = _disparity_head_args(x, weight, maps=(("y", y), ("d_y", d_y)))
    dev = x.device
    d_x = torch.empty_like(x) if need[0] else None
    d_w = torch.empty_like(weight) if need[1] else None
    d_b = torch.empty((1,), dtype=torch.float32, device=dev) if need[2] else None
    L = lib()
    ws = _entry_workspace(dev, L.mcr_disparity_head_backward_workspace_bytes, c_i64(B), c_i64(C), c_i64(Hs), c_i64(Ws))
    with torch.cuda.device(dev):
        check(L.mcr_disparity_head_backward(_p(x), _p(weight), _p(y), _p(d_y), _p(d_x) if need[0] else None, _p(d_w) if need[1] else None,
                                            _p(d_b) if need[2] else None, c_i64(B), c_int(C), c_int(Hs), c_int(Ws), _p(ws),
                                            c_size(ws.numel()), _stream()), "mcr_disparity_head_backward")
    return d_x, d_w, d_b


# ---- depth module: the expansion layers (transposed 3x3 conv + ELU, nearest resize, concat, reflect 3x3 conv + ELU) ----------------------
EXPANSION_LAYER_MAX_CHANNELS = 512


def _expansion_layer_shapes(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size, biases=True):
    """The shapes (ValueError, on any device) -> (B, Cin, Cmid, Cadd, Cout, h, w, H, W).  x [B,Cin,h,w], x_add [B,Cadd,H,W] or None,
    up_weight [Cin,Cmid,3,3], up_bias [Cmid], i_weight [Cout,Cmid+Cadd,3,3], i_bias [Cout], output_size (H, W); biases False: the
    backward, which reads none."""
    cap = EXPANSION_LAYER_MAX_CHANNELS
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"x must be [B,Cin,h,w], got {tuple(getattr(x, 'shape', ()))}")
    B, Cin, h, w = (int(v) for v in x.shape)
    try:
        H, W = (int(v) for v in output_size)
    except (TypeError, ValueError):
        raise ValueError(f"output_size must be a pair (H, W), got {output_size!r}") from None
    if B < 1 or not 1 <= Cin <= cap or h < 1 or w < 1:
        raise ValueError(f"x is {tuple(x.shape)}: B, h and w must be at least 1 and Cin between 1 and {cap}")
    if H < 2 or W < 2:
        raise ValueError(f"the output is {H} x {W}, H and W must be at least 2 (the reflection padding)")
    if not isinstance(up_weight, torch.Tensor) or up_weight.dim() != 4 or tuple(up_weight.shape[::3]) != (Cin, 3) or up_weight.shape[2] != 3:
        raise ValueError(f"up_weight must be [Cin,Cmid,3,3] with Cin = {Cin}, got {tuple(getattr(up_weight, 'shape', ()))}")
    Cmid = int(up_weight.shape[1])
    Cadd = 0
    if x_add is not None:
        if not isinstance(x_add, torch.Tensor) or x_add.dim() != 4 or (int(x_add.shape[0]), int(x_add.shape[2]), int(x_add.shape[3])) != (B, H, W):
            raise ValueError(f"x_add must be [B,Cadd,H,W] = [{B},Cadd,{H},{W}], got {tuple(getattr(x_add, 'shape', ()))}")
        Cadd = int(x_add.shape[1])
        if Cadd < 1:
            raise ValueError("x_add has no channels; pass None instead")
    if not 1 <= Cmid <= cap or Cmid + Cadd > cap:
        raise ValueError(f"Cmid = {Cmid} and Cadd = {Cadd}: Cmid must be between 1 and {cap} and Cmid + Cadd at most {cap}")
    if not isinstance(i_weight, torch.Tensor) or i_weight.dim() != 4 or tuple(i_weight.shape[1:]) != (Cmid + Cadd, 3, 3):
        raise ValueError(f"i_weight must be [Cout,Cmid+Cadd,3,3] with Cmid + Cadd = {Cmid + Cadd}, got {tuple(getattr(i_weight, 'shape', ()))}")
    Cout = int(i_weight.shape[0])
    if not 1 <= Cout <= cap:
        raise ValueError(f"Cout = {Cout} must be between 1 and {cap}")
    for name, t, n in (("up_bias", up_bias, Cmid), ("i_bias", i_bias, Cout)) if biases else ():
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n,):
            raise ValueError(f"{name} must be [{n}], got {tuple(getattr(t, 'shape', ()))}")
    if max(B * Cin * h * w, B * Cmid * h * w, B * Cadd * H * W, B * Cout * H * W) > 2 ** 31 - 1:
        raise ValueError(f"x is {tuple(x.shape)}, the output [{B},{Cout},{H},{W}]: a tensor has 2^31 elements or more")
    return B, Cin, Cmid, Cadd, Cout, h, w, H, W


def _expansion_layer_args(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size):
    """The shapes first (_expansion_layer_shapes), then the operands themselves (HIP, float32, contiguous)."""
    sizes = _expansion_layer_shapes(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size)
    ts = [_req(t, name) for name, t in (("x", x), ("up_weight", up_weight), ("up_bias", up_bias), ("i_weight", i_weight), ("i_bias", i_bias))]
    return ts, (_req(x_add, "x_add") if x_add is not None else None), sizes


def expansion_layer(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size, return_u=False):
    """y [B,Cout,H,W] = ELU(conv3x3(reflection_pad(cat(nearest(ELU(conv_transpose3x3(x, up_weight) + up_bias) -> output_size), x_add)),
    i_weight) + i_bias) in one entry (mcr_expansion_layer): upstream's ExpansionLayer.forward (ManyDepth.py:351-363).  x [B,Cin,h,w],
    x_add [B,Cadd,H,W] or None, the weights in upstream's layouts (upconv.weight [Cin,Cmid,3,3], iconv.weight [Cout,Cmid+Cadd,3,3]),
    float32.  Exact fp32 products; the same bits on every call.  return_u: (y, u) with u [B,Cmid,h,w] the transposed convolution after
    its ELU, which the backward reads -- the front of the entry's workspace, here a freshly allocated one instead of the shared arena
    that the next call overwrites."""
    (x, up_weight, up_bias, i_weight, i_bias), x_add, (B, Cin, Cmid, Cadd, Cout, h, w, H, W) = _expansion_layer_args(
        x, x_add, up_weight, up_bias, i_weight, i_bias, output_size)
    dev = x.device
    y = torch.empty((B, Cout, H, W), dtype=torch.float32, device=dev)
    L = lib()
    if return_u:
        nbytes = max(int(L.mcr_expansion_layer_workspace_bytes(c_i64(B), c_i64(Cmid), c_i64(h), c_i64(w))), 4 * B * Cmid * h * w)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = _entry_workspace(dev, L.mcr_expansion_layer_workspace_bytes, c_i64(B), c_i64(Cmid), c_i64(h), c_i64(w))
    with torch.cuda.device(dev):
        check(L.mcr_expansion_layer(_p(x), _p(x_add) if x_add is not None else None, _p(up_weight), _p(up_bias), _p(i_weight), _p(i_bias),
                                    _p(y), c_i64(B), c_int(Cin), c_int(Cmid), c_int(Cadd), c_int(Cout), c_int(h), c_int(w), c_int(H),
                                    c_int(W), _p(ws), c_size(ws.numel()), _stream()), "mcr_expansion_layer")
    if return_u:
        return y, ws[:4 * B * Cmid * h * w].view(torch.float32).view(B, Cmid, h, w)
    return y


def expansion_layer_backward(x, x_add, up_weight, i_weight, u, y, d_y, output_size, need=(True,) * 6):
    """(d_x, d_x_add, d_up_weight, d_up_bias, d_i_weight, d_i_bias) of sum(d_y * y) for y, u = expansion_layer(..., return_u=True), in one
    entry (mcr_expansion_layer_backward); u [B,Cmid,h,w], y and d_y [B,Cout,H,W].  need: which of the six are computed, the others are
    None; d_x_add is None without an x_add whatever need says; nothing left to compute is refused.  Each launch runs only if an output
    that is asked for depends on it.  No atomics: two calls give the same bits."""
    need = tuple(bool(n) for n in need)
    if len(need) != 6:
        raise ValueError("expansion_layer_backward: need names (d_x, d_x_add, d_up_weight, d_up_bias, d_i_weight, d_i_bias)")
    if x_add is None:
        need = (need[0], False) + need[2:]
    if not any(need):
        raise ValueError("expansion_layer_backward: need must name at least one of (d_x, d_x_add, d_up_weight, d_up_bias, d_i_weight, "
                         "d_i_bias); d_x_add counts only with an x_add")
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = _expansion_layer_shapes(x, x_add, up_weight, None, i_weight, None, output_size, biases=False)
    for name, t, shape in (("u", u, (B, Cmid, h, w)), ("y", y, (B, Cout, H, W)), ("d_y", d_y, (B, Cout, H, W))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
    if B * (Cmid + Cadd) * (H + 2) * (W + 2) > 2 ** 31 - 1:
        raise ValueError(f"the output [{B},{Cout},{H},{W}] with {Cmid + Cadd} concatenated channels: a tensor of the backward has 2^31 "
                         "elements or more")
    x, up_weight, i_weight = _req(x, "x"), _req(up_weight, "up_weight"), _req(i_weight, "i_weight")
    x_add = _req(x_add, "x_add") if x_add is not None else None
    u, y, d_y = _req(u, "u"), _req(y, "y"), _req(d_y, "d_y")
    dev = x.device
    shapes = ((B, Cin, h, w), (B, Cadd, H, W), (Cin, Cmid, 3, 3), (Cmid,), (Cout, Cmid + Cadd, 3, 3), (Cout,))
    outs = [torch.empty(shape, dtype=torch.float32, device=dev) if n else None for shape, n in zip(shapes, need)]
    L = lib()
    ws = _entry_workspace(dev, L.mcr_expansion_layer_backward_workspace_bytes, c_i64(B), c_i64(Cin), c_i64(Cmid), c_i64(Cadd), c_i64(Cout),
                          c_i64(h), c_i64(w), c_i64(H), c_i64(W))
    with torch.cuda.device(dev):
        check(L.mcr_expansion_layer_backward(_p(x), _p(x_add) if x_add is not None else None, _p(up_weight), _p(i_weight), _p(u), _p(y),
                                             _p(d_y), *[_p(o) if o is not None else None for o in outs], c_i64(B), c_int(Cin),
                                             c_int(Cmid), c_int(Cadd), c_int(Cout), c_int(h), c_int(w), c_int(H), c_int(W), _p(ws),
                                             c_size(ws.numel()), _stream()), "mcr_expansion_layer_backward")
    return tuple(outs)


# ---- depth module: the front of the ResNet encoder (7x7/2 conv + BatchNorm + ReLU + 3x3/2 max-pool; the basic blocks of layer1) ---------
RESNET_STEM_MAX_CIN = 8
RESNET_STEM_MAX_COUT = 64
BASIC_BLOCK_MAX_CHANNELS = 512
FEATURE_EXTRACTOR_MAX_BLOCKS = 4


def resnet_stem_sizes(H, W):
    """(Hc, Wc, Hp, Wp): the sizes of the stem's convolution (7x7, stride 2, padding 3) and of its max-pool (3x3, stride 2, padding 1)."""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Hc, Wc, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


def _bn_shapes(name, bn, C):
    """bn: (weight, bias, running_mean, running_var), each [C]."""
    if not isinstance(bn, (tuple, list)) or len(bn) != 4:
        raise ValueError(f"{name} must be (weight, bias, running_mean, running_var)")
    for part, t in zip(("weight", "bias", "running_mean", "running_var"), bn):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (C,):
            raise ValueError(f"{name}.{part} must be [{C}], got {tuple(getattr(t, 'shape', ()))}")


def _resnet_stem_shapes(x, x_more, weight, bias, bn):
    """The shapes (ValueError, on any device) -> (N0, N1, Cin, Cout, H, W).  x [N0,Cin,H,W] or None, x_more [N1,Cin,H,W] or None (not
    both), weight [Cout,Cin,7,7], bias [Cout] or None, bn the four vectors [Cout]."""
    first = x if x is not None else x_more
    if first is None:
        raise ValueError("x and x_more are both None: N0 + N1 must be at least 1")
    for name, t in (("x", x), ("x_more", x_more)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[1:]) != tuple(first.shape[1:])):
            raise ValueError(f"{name} must be [N,Cin,H,W] like the other image operand, got {tuple(getattr(t, 'shape', ()))}")
    N0, N1 = (0 if x is None else int(x.shape[0])), (0 if x_more is None else int(x_more.shape[0]))
    Cin, H, W = (int(v) for v in first.shape[1:])
    if N0 + N1 < 1 or H < 1 or W < 1 or not 1 <= Cin <= RESNET_STEM_MAX_CIN:
        raise ValueError(f"the images are [{N0}+{N1},{Cin},{H},{W}]: N0 + N1, H and W must be at least 1 and Cin between 1 and "
                         f"{RESNET_STEM_MAX_CIN}")
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or tuple(weight.shape[1:]) != (Cin, 7, 7):
        raise ValueError(f"weight must be [Cout,Cin,7,7] with Cin = {Cin}, got {tuple(getattr(weight, 'shape', ()))}")
    Cout = int(weight.shape[0])
    if not 1 <= Cout <= RESNET_STEM_MAX_COUT:
        raise ValueError(f"Cout = {Cout} must be between 1 and {RESNET_STEM_MAX_COUT}")
    if bias is not None and (not isinstance(bias, torch.Tensor) or tuple(bias.shape) != (Cout,)):
        raise ValueError(f"bias must be [{Cout}] or None, got {tuple(getattr(bias, 'shape', ()))}")
    _bn_shapes("bn", bn, Cout)
    Hc, Wc, _, _ = resnet_stem_sizes(H, W)
    if max((N0 + N1) * Cin * H * W, (N0 + N1) * Cout * Hc * Wc) > 2 ** 31 - 1:
        raise ValueError(f"the images are [{N0}+{N1},{Cin},{H},{W}], {Cout} output channels: a tensor has 2^31 elements or more")
    return N0, N1, Cin, Cout, H, W


def _basic_block_shapes(x, w1, bn1, w2, bn2, name="block"):
    """The shapes (ValueError, on any device) -> (B, C, H, W).  x [B,C,H,W], w1 and w2 [C,C,3,3], bn1 and bn2 the four vectors [C]."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"x must be [B,C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    B, C, H, W = (int(v) for v in x.shape)
    if B < 1 or H < 1 or W < 1 or not 1 <= C <= BASIC_BLOCK_MAX_CHANNELS:
        raise ValueError(f"x is {tuple(x.shape)}: B, H and W must be at least 1 and C between 1 and {BASIC_BLOCK_MAX_CHANNELS}")
    for wn, w in (("w1", w1), ("w2", w2)):
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != (C, C, 3, 3):
            raise ValueError(f"{name}.{wn} must be [{C},{C},3,3], got {tuple(getattr(w, 'shape', ()))}")
    _bn_shapes(f"{name}.bn1", bn1, C)
    _bn_shapes(f"{name}.bn2", bn2, C)
    if B * C * H * W > 2 ** 31 - 1:
        raise ValueError(f"x is {tuple(x.shape)}: a tensor has 2^31 elements or more")
    return B, C, H, W


def _req_bn(bn, name):
    return [_req(t, f"{name}.{part}") for part, t in zip(("weight", "bias", "running_mean", "running_var"), bn)]


def resnet_stem(x, x_more, weight, bias, bn, eps, want_conv1=True):
    """(pooled [N0+N1,Cout,Hp,Wp], conv1 [N0,Cout,Hc,Wc] or None) of max_pool2d(conv1, 3, 2, 1) with conv1 = relu(batch_norm(conv2d(
    image, weight [Cout,Cin,7,7], bias or None; stride 2, padding 3))), BatchNorm in eval mode (bn = (weight, bias, running_mean,
    running_var), eps), in one launch (mcr_resnet_stem): the front of upstream's FeatureExtractor.forward (ManyDepth.py:43-47) on the
    images of x [N0,Cin,H,W] and x_more [N1,Cin,H,W] (either may be None) without a concatenated copy.  conv1 is computed for x's images
    only, and only with want_conv1.  float32; exact fp32 products; the same bits on every call."""
    N0, N1, Cin, Cout, H, W = _resnet_stem_shapes(x, x_more, weight, bias, bn)
    x, x_more, bias = (None if t is None else _req(t, n) for n, t in (("x", x), ("x_more", x_more), ("bias", bias)))
    weight, bn = _req(weight, "weight"), _req_bn(bn, "bn")
    dev = weight.device
    Hc, Wc, Hp, Wp = resnet_stem_sizes(H, W)
    pooled = torch.empty((N0 + N1, Cout, Hp, Wp), dtype=torch.float32, device=dev)
    conv1 = torch.empty((N0, Cout, Hc, Wc), dtype=torch.float32, device=dev) if want_conv1 and N0 else None
    with torch.cuda.device(dev):
        check(lib().mcr_resnet_stem(*[None if t is None else _p(t) for t in (x, x_more, weight, bias, *bn)], c_f32(eps), _p(pooled),
                                    None if conv1 is None else _p(conv1), c_i64(N0), c_i64(N1), c_int(Cin), c_int(Cout), c_int(H), c_int(W),
                                    _stream()), "mcr_resnet_stem")
    return pooled, conv1


def basic_block(x, w1, bn1, eps1, w2, bn2, eps2, return_t=False):
    """y [B,C,H,W] = relu(batch_norm(conv2d(t, w2)) + x) with t = relu(batch_norm(conv2d(x, w1))), both convolutions 3 x 3, stride 1,
    padding 1, without bias, both BatchNorms in eval mode (bn = (weight, bias, running_mean, running_var)), in one entry
    (mcr_basic_block): torchvision's BasicBlock.forward without stride or downsample.  float32; exact fp32 products; the same bits on
    every call.  return_t: (y, t), t from a freshly allocated workspace instead of the shared arena."""
    B, C, H, W = _basic_block_shapes(x, w1, bn1, w2, bn2)
    x, w1, w2, bn1, bn2 = _req(x, "x"), _req(w1, "w1"), _req(w2, "w2"), _req_bn(bn1, "bn1"), _req_bn(bn2, "bn2")
    dev = x.device
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    L = lib()
    sizes = (c_i64(B), c_i64(C), c_i64(H), c_i64(W))
    if return_t:
        ws = torch.empty(max(int(L.mcr_basic_block_workspace_bytes(*sizes)), 4 * B * C * H * W), dtype=torch.uint8, device=dev)
    else:
        ws = _entry_workspace(dev, L.mcr_basic_block_workspace_bytes, *sizes)
    with torch.cuda.device(dev):
        check(L.mcr_basic_block(_p(x), _p(w1), *[_p(t) for t in bn1], c_f32(eps1), _p(w2), *[_p(t) for t in bn2], c_f32(eps2), _p(y),
                                c_i64(B), c_int(C), c_int(H), c_int(W), _p(ws), c_size(ws.numel()), _stream()), "mcr_basic_block")
    if return_t:
        return y, ws[:4 * B * C * H * W].view(torch.float32).view(B, C, H, W)
    return y


def feature_extractor(x, x_more, weight, bias, bn, eps, blocks, want_conv1=True):
    """(features [N0+N1,Cout,Hp,Wp], conv1 [N0,Cout,Hc,Wc] or None): resnet_stem followed by basic_block for every entry of `blocks`, a
    sequence of at most four (w1, bn1, eps1, w2, bn2, eps2), in one entry (mcr_feature_extractor, 1 + 2 len(blocks) launches): upstream's
    FeatureExtractor.forward (ManyDepth.py:43-50) on the images of x and x_more together, with the map after the first ReLU for x."""
    N0, N1, Cin, Cout, H, W = _resnet_stem_shapes(x, x_more, weight, bias, bn)
    blocks = list(blocks)
    if len(blocks) > FEATURE_EXTRACTOR_MAX_BLOCKS:
        raise ValueError(f"{len(blocks)} blocks, at most {FEATURE_EXTRACTOR_MAX_BLOCKS} are supported")
    Hc, Wc, Hp, Wp = resnet_stem_sizes(H, W)
    dev = weight.device
    pointers, eps_list, keep = [], [], []
    for k, blk in enumerate(blocks):
        w1, bn1, eps1, w2, bn2, eps2 = blk
        _basic_block_shapes(torch.empty((N0 + N1, Cout, Hp, Wp), device="meta"), w1, bn1, w2, bn2, name=f"blocks[{k}]")
        ts = [_req(w1, "w1"), *_req_bn(bn1, "bn1"), _req(w2, "w2"), *_req_bn(bn2, "bn2")]
        keep += ts
        pointers += [t.data_ptr() for t in ts]
        eps_list += [float(eps1), float(eps2)]
    x, x_more, bias = (None if t is None else _req(t, n) for n, t in (("x", x), ("x_more", x_more), ("bias", bias)))
    weight, bn = _req(weight, "weight"), _req_bn(bn, "bn")
    features = torch.empty((N0 + N1, Cout, Hp, Wp), dtype=torch.float32, device=dev)
    conv1 = torch.empty((N0, Cout, Hc, Wc), dtype=torch.float32, device=dev) if want_conv1 and N0 else None
    L = lib()
    ws = _entry_workspace(dev, L.mcr_feature_extractor_workspace_bytes, c_i64(N0), c_i64(N1), c_i64(Cin), c_i64(Cout), c_i64(H), c_i64(W),
                          c_i64(len(blocks)))
    ptr_array = (ctypes.c_void_p * max(len(pointers), 1))(*pointers)
    eps_array = (ctypes.c_float * max(len(eps_list), 1))(*eps_list)
    with torch.cuda.device(dev):
        check(L.mcr_feature_extractor(*[None if t is None else _p(t) for t in (x, x_more, weight, bias, *bn)], c_f32(eps), ptr_array,
                                      eps_array, c_int(len(blocks)), _p(features), None if conv1 is None else _p(conv1), c_i64(N0),
                                      c_i64(N1), c_int(Cin), c_int(Cout), c_int(H), c_int(W), _p(ws), c_size(ws.numel()), _stream()),
              "mcr_feature_extractor")
    return features, conv1
