"""The building-block C ABI (include/macarons_hip.h) on strided, offset and guarded operands.

Every other GPU test reaches these entry points through macarons_amd/ops.py, which packs every tensor (ld == row width) on a fresh
256-byte aligned allocation.  Here the calls go through ctypes on arenas (tests/_strided.py): operands with padding columns, moved
off the 16-byte grid, surrounded by a fill pattern.  Every case is compared with an fp64 CPU reference of the same operation, then
every element outside the output's logical window must still hold the fill bit for bit and every input must be unchanged.  For
aligned operands with ld % 4 == 0 the kernel choice does not depend on the leading dimension: the result must equal the packed
call's bit for bit.  Operands the header calls unsupported must be REFUSED: non-zero return, a message, the output untouched.

Tolerances are the project's: forward blocks |y - ref|.max() < 2e-5 * max(1, |ref|.max()) (test_linear_vs_numpy), backward blocks
BLOCK_TOL = 2e-5 on max|got - ref| / max|ref| per tensor (test_scone_vis_backward_gpu.py), column max bit-exact, mean 1e-6.
Every measured error is printed with the ERR prefix.

Last section: the five NETWORK entry points (PCTransformer, SconeVis forward and backward, SconeOcc dense and ragged, single call and
two phases) in a workspace of EXACTLY the bytes their size functions return, guarded on both sides, bit-equal to the call through
ops.* (which allocates 10 % more), and refused when the workspace is 4 bytes shorter.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _strided as st
from _strided import Arena, Workspace

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
BLOCK_TOL = 2e-5
I64, CI, VP, SZ = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


def L_():
    from macarons_amd import _lib
    return _lib.lib()


def stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def last_error():
    return L_().mcr_last_error().decode()


def P(a):
    return VP(a.ptr) if a is not None else VP(None)


def sync_ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {last_error()}"


def fwd_err(entry, tag, y, ref):
    e = float(np.abs(y.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"ERR {entry} {tag}: {e:.2e}")
    assert np.isfinite(y).all(), f"{entry} {tag}: non-finite output (an unwritten element keeps the fill)"
    assert e < FWD_TOL, f"{entry} {tag}: {e:.3e}"
    return e


def bwd_err(entry, tag, pairs):
    es = {k: st.rel_max(g, r) for k, (g, r) in pairs.items()}
    print(f"ERR {entry} {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in es.items()))
    for k, (g, _) in pairs.items():
        assert np.isfinite(g).all(), f"{entry} {tag}: non-finite {k}"
    assert max(es.values()) < BLOCK_TOL, f"{entry} {tag}: {es}"


def refused(rc, what, needle, outs):
    """The entry refused the call on the host: non-zero return, a message naming the reason, nothing written."""
    torch.cuda.synchronize()
    for o in outs:
        o.check_unchanged(f"{what}: output of a refused call")
    assert rc != 0, f"{what}: the call must be refused; it returned 0 and left the output untouched (message buffer: {last_error()!r})"
    assert needle in last_error(), f"{what}: message {last_error()!r} lacks {needle!r}"


# =====================================================================================================================================
# mcr_linear
# =====================================================================================================================================
# (ldx - K, ldy - N, ldr - N, offset X, offset Y, offset residual)
LIN_LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0), "pad4": (4, 4, 4, 0, 0, 0), "odd": (1, 3, 3, 0, 0, 0), "x+1": (0, 0, 0, 1, 0, 0),
               "y+1": (0, 0, 0, 0, 1, 0), "r+1": (0, 0, 0, 0, 0, 1), "all": (1, 3, 4, 1, 1, 1)}
# The branches of launch_linear (nn_kernels.hip), conditions taken from its code:
#   small-K vector kernel: K <= 4, N % 4 == 0, ldy % 4 == 0, Y aligned, M * N / 4 >= 65536   (its "odd" / "y+1" layouts drop to the generic kernel)
#   generic kernel, column tile nt: 8 -> halved while (nt / 2) * 32 >= N, then while cdiv(M, 128) * cdiv(N, nt * 32) < 512
#   deep_k: K >= 128, K % 4 == 0, cdiv(M, 128) * cdiv(N, 64) <= 512; nt 2 only when that product is exactly 512
#   split precision (linear3_applicable): K % 8 == 0, K >= 64, N >= 128, X / W aligned with ld % 4 == 0, cdiv(M, 128) * cdiv(N, 128) >= 256
LIN_SHAPES = [
    ("smallk_vec_k3", 2048, 128, 3), ("smallk_vec_k4", 2048, 128, 4), ("smallk_below", 2047, 128, 3), ("k4_n126", 130, 126, 4),
    ("one", 1, 1, 1), ("nt1", 1000, 125, 125), ("nt2", 16381, 200, 20), ("nt4", 32765, 200, 20), ("nt8", 65531, 200, 20),
    ("deep_nt1", 257, 512, 256), ("deep_nt1_n1", 300, 1, 256), ("deep_nt2", 16377, 256, 132),
    ("split_on", 32641, 128, 72), ("split_just_off", 32640, 128, 72), ("split_ragged", 40000, 200, 72),
]


def _lin_data(M, N, K):
    rng = np.random.default_rng(M + N + K)
    return (rng.standard_normal((M, K)).astype(np.float32), (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32),
            rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32))


def _run_linear(dev, x, w, b, r, gelu, layout, tag):
    (M, K), N = x.shape, w.shape[0]
    dx, dy, dr, ox, oy, orr = LIN_LAYOUTS[layout]
    X = Arena(M, K, K + dx, ox, x, dev)
    W = Arena(N, K, data=w, device=dev)
    B = Arena(1, N, data=b[None], device=dev) if b is not None else None
    R = Arena(M, N, N + dr, orr, r, dev) if r is not None else None
    Y = Arena(M, N, N + dy, oy, device=dev)
    rc = L_().mcr_linear(P(X), I64(X.ld), P(W), P(B), P(R), I64(R.ld if R else 0), P(Y), I64(Y.ld), I64(M), CI(N), CI(K), CI(int(gelu)),
                         stream())
    sync_ok(rc, tag)
    Y.check_guard(tag + " Y")
    for a in (X, W, B, R):
        if a is not None:
            a.check_unchanged(tag + " input")
    return Y.packed()


@pytest.mark.parametrize("name,M,N,K", LIN_SHAPES, ids=[s[0] for s in LIN_SHAPES])
def test_linear(dev, name, M, N, K):
    x, w, b, r = _lin_data(M, N, K)
    layouts = list(LIN_LAYOUTS) if M < 20000 else ["packed", "pad4", "odd", "all"]
    flag_sets = [(True, True, True), (False, False, False), (True, False, True), (False, True, False)] if M < 20000 else \
        [(True, True, True), (False, False, False)]
    for bias, gelu, res in flag_sets:
        ref = st.linear_ref(x, w, b if bias else None, gelu, r if res else None)
        packed = None
        for lay in layouts:
            tag = f"{name} M={M} N={N} K={K} bias={bias} gelu={gelu} res={res} {lay}"
            y = _run_linear(dev, x, w, b if bias else None, r if res else None, gelu, lay, tag)
            fwd_err("mcr_linear", tag, y, ref)
            if lay == "packed":
                packed = y
            elif lay == "pad4":          # aligned, ld % 4 == 0: no routing predicate of launch_linear reads more of ld than that
                assert np.array_equal(y.view(np.int32), packed.view(np.int32)), f"{tag}: differs from the packed call"


def test_linear_refuses_small_leading_dimensions(dev):
    x, w, b, r = _lin_data(8, 6, 5)
    X, W, R, Y = Arena(8, 5, data=x, device=dev), Arena(6, 5, data=w, device=dev), Arena(8, 6, data=r, device=dev), Arena(8, 6, device=dev)
    for ldx, ldr, ldy in ((4, 6, 6), (5, 5, 6), (5, 6, 5)):
        rc = L_().mcr_linear(P(X), I64(ldx), P(W), VP(None), P(R), I64(ldr), P(Y), I64(ldy), I64(8), CI(6), CI(5), CI(0), stream())
        refused(rc, f"mcr_linear ld {ldx, ldr, ldy}", "leading dimension too small", [Y])


# =====================================================================================================================================
# mcr_layernorm
# =====================================================================================================================================
LN_LAYOUTS = {"packed": (0, 0, 0, 0), "pad4": (4, 4, 0, 0), "odd": (1, 1, 0, 0), "x+1": (0, 0, 1, 0), "y+1": (0, 0, 0, 1), "all": (1, 4, 1, 1)}


@pytest.mark.parametrize("E", [1, 63, 64, 65, 126, 256, 512])
def test_layernorm(dev, E):
    rng = np.random.default_rng(E)
    g, b = rng.standard_normal(E).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    G, B = Arena(1, E, data=g[None], device=dev), Arena(1, E, data=b[None], device=dev)
    for M in (1, 3, 4, 5, 1000):          # four rows per block
        x = (rng.standard_normal((M, E)) * 3 + 1).astype(np.float32)
        ref = st.layernorm_ref(x, g, b)
        packed = None
        for lay, (dx, dy, ox, oy) in LN_LAYOUTS.items():
            tag = f"E={E} M={M} {lay}"
            X, Y = Arena(M, E, E + dx, ox, x, dev), Arena(M, E, E + dy, oy, device=dev)
            sync_ok(L_().mcr_layernorm(P(X), I64(X.ld), P(G), P(B), P(Y), I64(Y.ld), I64(M), CI(E), stream()), tag)
            Y.check_guard(tag)
            for a in (X, G, B):
                a.check_unchanged(tag)
            y = Y.packed()
            fwd_err("mcr_layernorm", tag, y, ref)
            if lay == "packed":
                packed = y
            elif lay == "pad4":
                assert np.array_equal(y.view(np.int32), packed.view(np.int32)), tag
    X, Y = Arena(4, E + 1, data=np.zeros((4, E + 1), np.float32), device=dev), Arena(4, E + 1, device=dev)
    if E > 1:
        for ldx, ldy in ((E - 1, E), (E, E - 1)):
            refused(L_().mcr_layernorm(P(X), I64(ldx), P(G), P(B), P(Y), I64(ldy), I64(4), CI(E), stream()), f"mcr_layernorm ld {ldx, ldy}",
                    "leading dimension too small", [Y])


# =====================================================================================================================================
# mcr_attention, mcr_attention_ws
# =====================================================================================================================================
HEADS = {"32x128": (4, 32, 128), "64x256": (4, 64, 256)}
# (ldq - W, ldo - v, offset qkv, offset out).  "q_odd" and "q+1" leave the MFMA kernel (al16 of launch_attention) for
# attention_flash_kernel, whose loads are scalar; every kernel writes `out` with scalar stores, so ldo / its offset are free.
ATT_LAYOUTS = {"packed": (0, 0, 0, 0), "pad4": (4, 4, 0, 0), "q_odd": (1, 0, 0, 0), "q+1": (0, 4, 1, 0), "o_odd+1": (0, 1, 0, 1)}
ATT_ALL = (1, 3, 1, 1)


def _qkv(S, L, W, seed):
    return np.random.default_rng(seed).standard_normal((S, L, W)).astype(np.float32)


def _attention_ref_chunked(qkv, H, qk, v, **kw):
    """The reference sequence by sequence (a [S, H, L, L] fp64 score tensor of the larger cases would not fit)."""
    S = qkv.shape[0]
    step = max(1, (1 << 24) // (H * qkv.shape[1] ** 2))
    out = []
    for s0 in range(0, S, step):
        k2 = {k: (None if a is None else np.asarray(a)[s0:s0 + step]) for k, a in kw.items()}
        out.append(st.attention_ref(qkv[s0:s0 + step], H, qk, v, **k2))
    return np.concatenate(out)


def _run_attention(dev, qkv, H, qk, v, layout, tag, with_ws):
    S, L, W = qkv.shape
    dq, do, oq, oo = ATT_LAYOUTS[layout] if isinstance(layout, str) else layout
    Q = Arena(S * L, W, W + dq, oq, qkv.reshape(S * L, W), dev)
    O = Arena(S * L, v, v + do, oo, device=dev)
    if with_ws:
        ws = Workspace(int(L_().mcr_attention_workspace_bytes(I64(S), I64(L), CI(H), CI(v))), dev)
        rc = L_().mcr_attention_ws(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v), P(ws), SZ(ws.n_bytes), stream())
    else:
        rc = L_().mcr_attention(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v), stream())
    sync_ok(rc, tag)
    O.check_guard(tag + " out")
    Q.check_unchanged(tag + " qkv")
    if with_ws:
        ws.check_guard(tag + " workspace")
    return O.packed().reshape(S, L, v)


# L = 16 on the (32,128) layout: attention_small_kernel, four sequences per block; on (64,256) the MFMA kernel.  Longer: the MFMA
# kernel; with a workspace its key-split form when L >= 512 and cdiv(L, 64) * H * S <= 256; its 128-query form when
# cdiv(L, 128) * H * S >= 512 ((43, 333)).
ATT_CASES = [("32x128", S, 16) for S in (1, 3, 4, 5)] + [("64x256", 5, 16)] + \
            [(h, S, L) for h in HEADS for (S, L) in ((2, 17), (2, 65), (3, 333), (1, 2048), (3, 2048), (43, 333))]


@pytest.mark.parametrize("heads,S,L", ATT_CASES)
def test_attention(dev, heads, S, L):
    H, qk, v = HEADS[heads]
    qkv = _qkv(S, L, 2 * qk + v, S * 1000 + L)
    ref = _attention_ref_chunked(qkv, H, qk, v)
    for with_ws in (False, True):
        entry = "mcr_attention_ws" if with_ws else "mcr_attention"
        packed = None
        for lay in ATT_LAYOUTS:
            flash = lay in ("q_odd", "q+1") and not (L == 16 and heads == "32x128")
            tag = f"{heads} S={S} L={L} {lay}" + (" [attention_flash_kernel]" if flash else "")
            y = _run_attention(dev, qkv, H, qk, v, lay, f"{entry} {tag}", with_ws)
            fwd_err(entry, tag, y, ref)
            if lay == "packed":
                packed = y
            elif lay in ("pad4", "o_odd+1"):       # same kernel, same aligned qkv: only where the rows land differs
                assert np.array_equal(y.view(np.int32), packed.view(np.int32)), f"{entry} {tag}: differs from the packed call"


def test_attention_more_than_65535_short_sequences(dev):
    """S = 70000 sequences of 16 tokens (attention_small_kernel's grid is S / 4 blocks), odd leading dimensions, both operands offset."""
    H, qk, v = HEADS["32x128"]
    S, L = 70000, 16
    qkv = _qkv(S, L, 2 * qk + v, 7)
    ref = _attention_ref_chunked(qkv, H, qk, v)
    y = _run_attention(dev, qkv, H, qk, v, ATT_ALL, "mcr_attention S=70000", False)
    fwd_err("mcr_attention", "32x128 S=70000 L=16 all", y, ref)


def test_attention_refuses_small_leading_dimensions(dev):
    H, qk, v = HEADS["32x128"]
    Q, O = Arena(34, 192, data=_qkv(2, 17, 192, 0).reshape(34, 192), device=dev), Arena(34, 128, device=dev)
    ws = Workspace(int(L_().mcr_attention_workspace_bytes(I64(2), I64(17), CI(H), CI(v))), dev)
    for ldq, ldo in ((191, 128), (192, 127)):
        refused(L_().mcr_attention(P(Q), I64(ldq), P(O), I64(ldo), I64(2), I64(17), CI(H), CI(qk), CI(v), stream()), "mcr_attention",
                "leading dimension too small", [O])
        refused(L_().mcr_attention_ws(P(Q), I64(ldq), P(O), I64(ldo), I64(2), I64(17), CI(H), CI(qk), CI(v), P(ws), SZ(ws.n_bytes), stream()),
                "mcr_attention_ws", "leading dimension too small", [O])


# =====================================================================================================================================
# mcr_attention_masked
# =====================================================================================================================================
def _mask(kind, S, H, L, seed):
    """(bytes [..], seq / head / query strides, the bool mask broadcastable to [S, H, L, L])."""
    rng = np.random.default_rng(seed)
    if kind == "pair":
        m = rng.random((S, 1, L, L)) < 0.7
        m[0, 0, min(3, L - 1), :] = False                      # a fully masked query: uniform attention (-1e3, not -inf)
        return m.astype(np.uint8), (L * L, 0, L), m
    if kind == "key":
        m = rng.random((S, 1, 1, L)) < 0.7
        m[..., 0] = True
        return m.astype(np.uint8), (L, 0, 0), m
    m = rng.random((S, H, L, L)) < 0.7                         # per head
    m[S - 1, H - 1, 0, :] = False
    return m.astype(np.uint8), (H * L * L, L * L, L), m


def _call_masked(dev, Q, O, S, L, H, qk, v, mbytes, strides, ws):
    mt = torch.from_numpy(mbytes.reshape(-1).copy()).to(dev)
    rc = L_().mcr_attention_masked(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v), VP(mt.data_ptr()), I64(strides[0]),
                                   I64(strides[1]), I64(strides[2]), P(ws), SZ(ws.n_bytes if ws else 0), stream())
    torch.cuda.synchronize()
    assert np.array_equal(mt.cpu().numpy(), mbytes.reshape(-1)), "the mask changed"
    return rc


@pytest.mark.parametrize("kind", ["pair", "key", "head"])
@pytest.mark.parametrize("heads,S,L", [("32x128", 5, 16), ("64x256", 3, 16), ("32x128", 2, 65), ("64x256", 2, 65), ("32x128", 2, 333),
                                       ("64x256", 1, 333), ("32x128", 1, 600)])        # (1, 600) with a workspace: the key-split form
def test_attention_masked(dev, kind, heads, S, L):
    H, qk, v = HEADS[heads]
    W = 2 * qk + v
    qkv = _qkv(S, L, W, S * 100 + L)
    mbytes, strides, mbool = _mask(kind, S, H, L, L)
    ref = st.attention_ref(qkv, H, qk, v, mask=mbool)
    small = L == 16 and heads == "32x128"       # attention_small_kernel: taken before the alignment test, scalar loads: any ldq / offset
    packed = None
    for lay, (dq, do, oq, oo) in ATT_LAYOUTS.items():
        tag = f"{kind} {heads} S={S} L={L} {lay}"
        Q = Arena(S * L, W, W + dq, oq, qkv.reshape(S * L, W), dev)
        O = Arena(S * L, v, v + do, oo, device=dev)
        ws = Workspace(int(L_().mcr_attention_workspace_bytes(I64(S), I64(L), CI(H), CI(v))), dev) if L >= 512 else None
        rc = _call_masked(dev, Q, O, S, L, H, qk, v, mbytes, strides, ws)
        if lay in ("q_odd", "q+1") and not small:
            # the masked form exists on the MFMA kernel alone (16-byte loads): the header asks for ldq % 4 == 0 and an aligned qkv
            refused(rc, "mcr_attention_masked " + tag, "launch_attention: per-sequence lengths / masks need the MFMA kernel", [O])
            print(f"REFUSED mcr_attention_masked {tag}")
            continue
        sync_ok(rc, tag)
        O.check_guard(tag)
        Q.check_unchanged(tag)
        if ws:
            ws.check_guard(tag + " workspace")
        y = O.packed().reshape(S, L, v)
        fwd_err("mcr_attention_masked", tag, y, ref)
        if lay == "packed":
            packed = y
        elif lay in ("pad4", "o_odd+1"):
            assert np.array_equal(y.view(np.int32), packed.view(np.int32)), tag


# =====================================================================================================================================
# mcr_attention_planes
# =====================================================================================================================================
@pytest.mark.parametrize("split_mode", [1, 0, -1])
@pytest.mark.parametrize("heads,S,L,lens", [("32x128", 2, 700, None), ("32x128", 3, 700, [1, 350, 700]), ("64x256", 1, 1100, None),
                                            ("64x256", 2, 1100, [517, 1]), ("32x128", 2, 520, [520, 7])])
def test_attention_planes(dev, split_mode, heads, S, L, lens):
    H, qk, v = HEADS[heads]
    W = 2 * qk + v
    qkv = _qkv(S, L, W, S * 10 + L)
    ref = _attention_ref_chunked(qkv, H, qk, v, lens=lens)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    nb = int(L_().mcr_attention_planes_workspace_bytes(I64(S), I64(L), CI(H), CI(qk), CI(v)))

    def call(Q, O, ws, ldq=None):
        return L_().mcr_attention_planes(P(Q), I64(ldq or Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v),
                                         VP(lt.data_ptr() if lt is not None else None), CI(split_mode), P(ws), SZ(ws.n_bytes), stream())

    packed = None
    for lay, (dq, do, oq, oo) in {"packed": (0, 0, 0, 0), "pad4": (4, 4, 0, 0), "o_odd+1": (0, 1, 0, 1)}.items():
        tag = f"{heads} S={S} L={L} lens={lens} split_mode={split_mode} {lay}"
        Q, O, ws = Arena(S * L, W, W + dq, oq, qkv.reshape(S * L, W), dev), Arena(S * L, v, v + do, oo, device=dev), Workspace(nb, dev)
        sync_ok(call(Q, O, ws), tag)
        O.check_guard(tag)
        ws.check_guard(tag + " workspace")
        Q.check_unchanged(tag)
        y = O.packed().reshape(S, L, v)
        fwd_err("mcr_attention_planes", tag, y, ref)       # two-term fp16 split of q, k, v (22 significant bits): inside the fp32 bound
        if lay == "packed":
            packed = y
        else:
            assert np.array_equal(y.view(np.int32), packed.view(np.int32)), tag
    if split_mode != 1:
        return
    # split_to_planes_kernel reads every row in 16-byte groups, the planes are read by 16-byte DMA: the header asks for ldq % 4 == 0,
    # qkv and workspace 16-byte aligned
    O = Arena(S * L, v, device=dev)
    for what, Q, ws in (("ldq = W + 1", Arena(S * L, W, W + 1, 0, qkv.reshape(S * L, W), dev), Workspace(nb, dev)),
                        ("qkv + 1 float", Arena(S * L, W, W, 1, qkv.reshape(S * L, W), dev), Workspace(nb, dev)),
                        ("workspace + 1 float", Arena(S * L, W, W, 0, qkv.reshape(S * L, W), dev), Workspace(nb, dev, offset=1))):
        refused(call(Q, O, ws), f"mcr_attention_planes {what}", "ldq must be a multiple of 4, qkv and workspace 16-byte aligned", [O, ws])
        print(f"REFUSED mcr_attention_planes {heads} {what}")
    Q, ws = Arena(S * L, W, data=qkv.reshape(S * L, W), device=dev), Workspace(nb, dev)
    refused(call(Q, O, ws, ldq=W - 4), "mcr_attention_planes ldq < W", "leading dimension too small", [O, ws])


# =====================================================================================================================================
# mcr_colmax_broadcast, mcr_pool_max_avg
# =====================================================================================================================================
POOL_LAYOUTS = {"packed": (0, 0, 0, 0), "pad4": (4, 4, 0, 0), "odd": (1, 1, 0, 0), "x+1": (0, 0, 1, 0), "y+1": (0, 4, 0, 1), "all": (1, 1, 1, 1)}


@pytest.mark.parametrize("E", [1, 63, 64, 65, 126, 250])
@pytest.mark.parametrize("S,L", [(3, 1), (2, 17), (3, 511), (3, 512), (1, 600)])     # pool_kernel below 512 rows, pool_long_kernel from 512
def test_colmax_and_pool(dev, S, L, E):
    x = np.random.default_rng(S * L + E).standard_normal((S, L, E)).astype(np.float32)
    mx, mean = x.max(1), x.astype(np.float64).mean(1)
    for lay, (dx, dy, ox, oy) in POOL_LAYOUTS.items():
        tag = f"S={S} L={L} E={E} {lay}"
        X = Arena(S * L, E, E + dx, ox, x.reshape(S * L, E), dev)
        Y = Arena(S * L, E, E + dy, oy, device=dev)
        sync_ok(L_().mcr_colmax_broadcast(P(X), I64(X.ld), P(Y), I64(Y.ld), I64(S), I64(L), CI(E), stream()), "colmax " + tag)
        Y.check_guard("colmax " + tag)
        X.check_unchanged("colmax " + tag)
        assert np.array_equal(Y.packed().reshape(S, L, E).view(np.int32), np.broadcast_to(mx[:, None], x.shape).view(np.int32)), "colmax " + tag
        Z = Arena(S, 2 * E, 2 * E + dy, oy, device=dev)
        sync_ok(L_().mcr_pool_max_avg(P(X), I64(X.ld), P(Z), I64(Z.ld), I64(S), I64(L), CI(E), stream()), "pool " + tag)
        Z.check_guard("pool " + tag)
        X.check_unchanged("pool " + tag)
        z = Z.packed()
        assert np.array_equal(z[:, :E].view(np.int32), mx.view(np.int32)), "pool max " + tag
        e = float(np.abs(z[:, E:] - mean).max())
        print(f"ERR mcr_pool_max_avg mean {tag}: {e:.2e}")
        assert e < 1e-6, tag
    if E > 1:
        X, Y = Arena(S * L, E, data=x.reshape(S * L, E), device=dev), Arena(S * L, 2 * E, device=dev)
        for ldx, ldy in ((E - 1, E), (E, E - 1)):
            refused(L_().mcr_colmax_broadcast(P(X), I64(ldx), P(Y), I64(ldy), I64(S), I64(L), CI(E), stream()), "mcr_colmax_broadcast",
                    "leading dimension too small", [Y])
        for ldx, ldy in ((E - 1, 2 * E), (E, 2 * E - 1)):
            refused(L_().mcr_pool_max_avg(P(X), I64(ldx), P(Y), I64(ldy), I64(S), I64(L), CI(E), stream()), "mcr_pool_max_avg",
                    "leading dimension too small", [Y])


# =====================================================================================================================================
# mcr_attention_backward
# =====================================================================================================================================
# ab_nsplit(S, L, H) = 1 when S * H * cdiv(L, 64) >= 512, 2 from 256, else 4.  With H = 4: (16, 256) is 256 blocks, (15, 256) and
# (16, 192) are below it, (16, 257) above; (32, 256) is 512, (31, 256) and (32, 192) below it.
AB_CASES = [(1, 2048), (4, 2048), (3, 333), (2, 17), (16, 256), (15, 256), (16, 192), (16, 257), (32, 256), (31, 256), (32, 192)]


def _ab_ref(qkv, g, lens):
    return np.concatenate([st.attention_backward_ref(qkv[s:s + 1], g[s:s + 1], 4, 64, 256, None if lens is None else lens[s:s + 1])
                           for s in range(qkv.shape[0])])


def _ab_call(Q, G, D, S, L, lt, ws, lds=None):
    ldq, ldg, ldd = lds or (Q.ld, G.ld, D.ld)
    return L_().mcr_attention_backward(P(Q), I64(ldq), P(G), I64(ldg), P(D), I64(ldd), I64(S), I64(L), CI(4), CI(64), CI(256),
                                       VP(lt.data_ptr() if lt is not None else None), P(ws), SZ(ws.n_bytes), stream())


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("S,L", AB_CASES)
def test_attention_backward(dev, S, L, with_lens):
    rng = np.random.default_rng(S * 1000 + L)
    qkv = rng.standard_normal((S, L, 384)).astype(np.float32)
    g = rng.standard_normal((S, L, 256)).astype(np.float32)
    lens = np.array(([1] + [max(1, L // 2 - 3)] * (S - 1))[:S] if S > 1 else [L // 3], np.int32) if with_lens else None
    lt = torch.from_numpy(lens).to(dev) if with_lens else None
    ref = _ab_ref(qkv, g, lens)
    nb = int(L_().mcr_attention_backward_workspace_bytes(I64(S), I64(L), CI(4), CI(256)))
    packed = None
    # each leading dimension at its width and at width + 4 (the kernels use 16-byte accesses: nothing else is accepted)
    for pads in [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 8, 12)]:
        tag = f"S={S} L={L} lens={with_lens} ld+{pads}"
        Q = Arena(S * L, 384, 384 + pads[0], 0, qkv.reshape(-1, 384), dev)
        G = Arena(S * L, 256, 256 + pads[1], 0, g.reshape(-1, 256), dev)
        D = Arena(S * L, 384, 384 + pads[2], 0, device=dev)
        ws = Workspace(nb, dev)
        sync_ok(_ab_call(Q, G, D, S, L, lt, ws), tag)
        D.check_guard(tag)
        ws.check_guard(tag + " workspace")
        Q.check_unchanged(tag)
        G.check_unchanged(tag)
        d = D.packed().reshape(S, L, 384)
        bwd_err("mcr_attention_backward", tag, {"dq": (d[..., :64], ref[..., :64]), "dk": (d[..., 64:128], ref[..., 64:128]),
                                                 "dv": (d[..., 128:], ref[..., 128:])})
        if with_lens:
            for s in range(S):           # keys beyond the length: exact zeros
                assert not d[s, int(lens[s]):, 64:].any(), tag
        if packed is None:
            packed = d
        else:
            assert np.array_equal(d.view(np.int32), packed.view(np.int32)), f"{tag}: differs from the packed call"


def test_attention_backward_refuses_what_the_header_excludes(dev):
    S, L = 2, 17
    rng = np.random.default_rng(0)
    qkv, g = rng.standard_normal((S * L, 384)).astype(np.float32), rng.standard_normal((S * L, 256)).astype(np.float32)
    nb = int(L_().mcr_attention_backward_workspace_bytes(I64(S), I64(L), CI(4), CI(256)))
    mk = lambda pq=0, pg=0, pd=0, oq=0, og=0, od=0, ow=0: (Arena(S * L, 384, 384 + pq, oq, qkv, dev), Arena(S * L, 256, 256 + pg, og, g, dev),
                                                            Arena(S * L, 384, 384 + pd, od, device=dev), Workspace(nb, dev, offset=ow))
    for kw, needle in (({"pq": 1}, "multiples of 4"), ({"pg": 1}, "multiples of 4"), ({"pd": 1}, "multiples of 4"),
                       ({"oq": 1}, "16-byte aligned"), ({"og": 1}, "16-byte aligned"), ({"od": 1}, "16-byte aligned"),
                       ({"ow": 1}, "workspace must be 16-byte aligned")):
        Q, G, D, ws = mk(**kw)
        refused(_ab_call(Q, G, D, S, L, None, ws), f"mcr_attention_backward {kw}", needle, [D, ws])
        print(f"REFUSED mcr_attention_backward {kw}")
    Q, G, D, ws = mk()
    for lds in ((380, 256, 384), (384, 252, 384), (384, 256, 380)):
        refused(_ab_call(Q, G, D, S, L, None, ws, lds), f"mcr_attention_backward ld {lds}", "leading dimensions must cover the rows", [D, ws])


# =====================================================================================================================================
# mcr_linear_backward
# =====================================================================================================================================
# (ldx - K, ldz - N, ldy - N, ld_dx - K, offsets X, Z, dY, dX).  Every kernel behind this entry loads and stores scalars (the dX GEMM
# is launch_linear, whose 16-byte loads sit behind vec_x / vec_w): odd leading dimensions and offset operands are supported.
LB_LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0, 0, 0), "pad4": (4, 4, 4, 4, 0, 0, 0, 0), "odd": (1, 1, 1, 1, 0, 0, 0, 0),
              "offsets": (0, 0, 0, 0, 1, 1, 1, 1), "all": (1, 4, 1, 4, 1, 0, 1, 1)}


def _lb_data(M, N, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, K)).astype(np.float32), (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32),
            (rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32),
            rng.standard_normal((M, K)).astype(np.float32))


def _lb_run(dev, data, ref, gelu, acc, layout, want, tag):
    """want: which of (dX, dW, db) are asked for; the others are passed as NULL and their arenas must stay untouched."""
    x, w, b, g, base = data
    (M, K), N = x.shape, w.shape[0]
    rdx, rdw, rdb, z = ref
    px, pz, py, pd, ox, oz, oy, od = LB_LAYOUTS[layout]
    X, W = Arena(M, K, K + px, ox, x, dev), Arena(N, K, data=w, device=dev)
    Z = Arena(M, N, N + pz, oz, z.astype(np.float32), dev) if gelu else None
    G = Arena(M, N, N + py, oy, g, dev)
    DX = Arena(M, K, K + pd, od, base if acc else None, dev)
    DW, DB = Arena(N, K, device=dev), Arena(1, N, device=dev)
    ws = Workspace(int(L_().mcr_linear_backward_workspace_bytes(I64(M), CI(N), CI(K))), dev)
    rc = L_().mcr_linear_backward(P(X), I64(X.ld), P(W), P(Z), I64(Z.ld if Z else 0), P(G), I64(G.ld), I64(M), CI(N), CI(K), CI(int(gelu)),
                                  P(DX if want[0] else None), I64(DX.ld), CI(int(acc)), P(DW if want[1] else None),
                                  P(DB if want[2] else None), P(ws), SZ(ws.n_bytes), stream())
    sync_ok(rc, tag)
    for a in (X, W, Z, G):
        if a is not None:
            a.check_unchanged(tag + " input")
    ws.check_guard(tag + " workspace")
    pairs, bits = {}, {}
    for name, arena, asked, r in (("dx", DX, want[0], rdx + (base if acc else 0)), ("dw", DW, want[1], rdw), ("db", DB, want[2], rdb[None])):
        if asked:
            arena.check_guard(f"{tag} {name}")
            pairs[name] = bits[name] = (arena.packed(), r)
        else:
            arena.check_unchanged(f"{tag} {name} (not asked for)")
    if pairs:
        bwd_err("mcr_linear_backward", tag, pairs)
    return {k: v[0] for k, v in bits.items()}


# SconeVis's layers (mcr_scone_vis_backward: embedding 4 -> 126 -> 126; encoders qkv 256 -> 384, out 256 -> 256, ff 256 -> 512 -> 256;
# head 256 -> 192 -> 128 -> 64, fc2 reading 256 = 192 + the view harmonics), then the edges
LB_SHAPES = [(777, 126, 4), (777, 126, 126), (777, 384, 256), (300, 256, 256), (300, 512, 256), (300, 256, 512), (777, 192, 256),
             (777, 128, 256), (777, 64, 128), (1, 7, 5), (50, 1, 9), (50, 9, 1), (130, 65, 4), (515, 100, 70)]


@pytest.mark.parametrize("M,N,K", LB_SHAPES)
def test_linear_backward_shapes_and_layouts(dev, M, N, K):
    data = _lb_data(M, N, K, M + N + K)
    for gelu in (False, True):
        ref = st.linear_backward_ref(data[0], data[1], data[2], data[3], gelu)
        for acc in (False, True):
            packed = None
            for lay in LB_LAYOUTS:
                out = _lb_run(dev, data, ref, gelu, acc, lay, (True, True, True), f"M={M} N={N} K={K} gelu={gelu} acc={acc} {lay}")
                if lay == "packed":
                    packed = out
                elif lay == "pad4":
                    for k in out:
                        assert np.array_equal(out[k].view(np.int32), packed[k].view(np.int32)), f"{k} {lay}: differs from the packed call"


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("acc", [False, True])
def test_linear_backward_every_subset_of_outputs(dev, gelu, acc):
    M, N, K = 300, 20, 12
    data = _lb_data(M, N, K, 3)
    ref = st.linear_backward_ref(data[0], data[1], data[2], data[3], gelu)
    full = _lb_run(dev, data, ref, gelu, acc, "odd", (True, True, True), "all three")
    for want in itertools.product((False, True), repeat=3):
        out = _lb_run(dev, data, ref, gelu, acc, "odd", want, f"gelu={gelu} acc={acc} outputs (dX, dW, db)={want}")
        for k in out:                                            # the outputs asked for keep their bits
            assert np.array_equal(out[k].view(np.int32), full[k].view(np.int32)), (k, want)


def test_linear_backward_slab_boundaries(dev):
    """dW / db are summed over vb_slabs(M) = cdiv(M, max(256, 16 * cdiv(cdiv(M, 64), 16))) slabs of rows: up to 16384 rows a slab is
    256 rows, so the count changes at every multiple of 256.  M either side of each change up to 4 x 2048 rows; every row of dY
    carries weight (a slab dropped or read twice moves db by ~1 / sqrt(M), far above the bound)."""
    N, K = 5, 6
    for M in sorted({m + d for m in range(256, 4 * 2048 + 1, 256) for d in (0, 1)} | {255}):
        data = _lb_data(M, N, K, M)
        ref = st.linear_backward_ref(data[0], data[1], data[2], data[3], False)
        _lb_run(dev, data, ref, False, False, "all" if M % 512 else "packed", (True, True, True), f"slabs M={M}")
    for M in (16384, 16385, 40000):                              # past 16384 rows the slabs grow instead (at most 64 of them)
        data = _lb_data(M, N, K, M)
        ref = st.linear_backward_ref(data[0], data[1], data[2], data[3], True)
        _lb_run(dev, data, ref, True, True, "odd", (True, True, True), f"slabs M={M}")


def test_linear_backward_refuses_small_leading_dimensions(dev):
    M, N, K = 20, 8, 6
    x, w, b, g, base = _lb_data(M, N, K, 0)
    X, W, Z, G = Arena(M, K, data=x, device=dev), Arena(N, K, data=w, device=dev), Arena(M, N, data=g, device=dev), Arena(M, N, data=g, device=dev)
    DX, DW, DB = Arena(M, K, device=dev), Arena(N, K, device=dev), Arena(1, N, device=dev)
    ws = Workspace(int(L_().mcr_linear_backward_workspace_bytes(I64(M), CI(N), CI(K))), dev)
    for ldx, ldz, ldy, ldd in ((K - 1, N, N, K), (K, N - 1, N, K), (K, N, N - 1, K), (K, N, N, K - 1)):
        rc = L_().mcr_linear_backward(P(X), I64(ldx), P(W), P(Z), I64(ldz), P(G), I64(ldy), I64(M), CI(N), CI(K), CI(1), P(DX), I64(ldd), CI(0),
                                      P(DW), P(DB), P(ws), SZ(ws.n_bytes), stream())
        refused(rc, f"mcr_linear_backward ld {ldx, ldz, ldy, ldd}", "leading dimension too small", [DX, DW, DB, ws])


def test_linear_backward_needs_x_for_db_as_well_as_for_dw(dev):
    """db rides on the dW product, which reads X: the header allows X == NULL only when neither is asked for."""
    M, N, K = 20, 8, 6
    x, w, b, g, base = _lb_data(M, N, K, 1)
    ref = st.linear_backward_ref(x, w, b, g, False)
    W, G = Arena(N, K, data=w, device=dev), Arena(M, N, data=g, device=dev)
    DX, DW, DB = Arena(M, K, device=dev), Arena(N, K, device=dev), Arena(1, N, device=dev)
    ws = Workspace(int(L_().mcr_linear_backward_workspace_bytes(I64(M), CI(N), CI(K))), dev)
    call = lambda dx, dw, db: L_().mcr_linear_backward(VP(None), I64(K), P(W), VP(None), I64(0), P(G), I64(N), I64(M), CI(N), CI(K), CI(0), P(dx),
                                                        I64(K), CI(0), P(dw), P(db), P(ws), SZ(ws.n_bytes), stream())
    refused(call(DX, None, DB), "mcr_linear_backward X == NULL with db", "null pointer", [DX, DW, DB, ws])
    refused(call(DX, DW, None), "mcr_linear_backward X == NULL with dW", "null pointer", [DX, DW, DB, ws])
    sync_ok(call(DX, None, None), "X == NULL, dX alone")
    DX.check_guard("dX alone")
    for a in (DW, DB, W, G):
        a.check_unchanged("dX alone")
    bwd_err("mcr_linear_backward", "X == NULL, dX alone", {"dx": (DX.packed(), ref[0])})


# =====================================================================================================================================
# mcr_layernorm_backward
# =====================================================================================================================================
# (ldx - E, ldy - E, ld_dx - E, offsets X, dY, dX): scalar loads and stores throughout
LNB_LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0), "pad4": (4, 4, 4, 0, 0, 0), "odd": (1, 1, 1, 0, 0, 0), "offsets": (0, 0, 0, 1, 1, 1),
               "all": (1, 4, 1, 1, 0, 1)}
# d_gamma / d_beta are summed over cdiv(M, vb_ln_rows(M)) blocks, vb_ln_rows(M) = max(16, 4 * cdiv(cdiv(M, 256), 4)): 16 rows up to
# M = 4096 (the count changes at every multiple of 16: the first ones, one in the middle, the last), 20 rows from 4097.
LNB_M = [1, 5, 15, 16, 17, 31, 32, 33, 999, 1008, 1009, 4080, 4081, 4096, 4097, 5000]


@pytest.mark.parametrize("E", [64, 128, 256, 512])
def test_layernorm_backward(dev, E):
    rng = np.random.default_rng(9 + E)
    gm = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    GM = Arena(1, E, data=gm[None], device=dev)
    for M in LNB_M:
        x = (rng.standard_normal((M, E)) * 2 + 0.5).astype(np.float32)
        g = rng.standard_normal((M, E)).astype(np.float32)
        base = rng.standard_normal((M, E)).astype(np.float32)
        rdx, rdg, rdb = st.layernorm_backward_ref(x, gm, g)
        ws_bytes = int(L_().mcr_layernorm_backward_workspace_bytes(I64(M), CI(E)))
        layouts = list(LNB_LAYOUTS) if M in (5, 33, 1009) else ["packed" if M % 2 else "all"]
        packed = None
        for lay in layouts:
            px, py, pd, ox, oy, od = LNB_LAYOUTS[lay]
            for acc, want_g, want_b in ((False, True, True), (True, True, True), (False, False, True), (True, True, False), (False, False, False)):
                tag = f"E={E} M={M} {lay} acc={acc} d_gamma={want_g} d_beta={want_b}"
                X, G = Arena(M, E, E + px, ox, x, dev), Arena(M, E, E + py, oy, g, dev)
                DX = Arena(M, E, E + pd, od, base if acc else None, dev)
                DG, DB, ws = Arena(1, E, device=dev), Arena(1, E, device=dev), Workspace(ws_bytes, dev)
                rc = L_().mcr_layernorm_backward(P(X), I64(X.ld), P(GM), P(G), I64(G.ld), I64(M), CI(E), P(DX), I64(DX.ld), CI(int(acc)),
                                                 P(DG if want_g else None), P(DB if want_b else None), P(ws), SZ(ws.n_bytes), stream())
                sync_ok(rc, tag)
                for a in (X, G, GM):
                    a.check_unchanged(tag)
                DX.check_guard(tag)
                ws.check_guard(tag + " workspace")
                pairs = {"dx": (DX.packed(), rdx + (base if acc else 0))}
                for name, arena, asked, r in (("dgamma", DG, want_g, rdg), ("dbeta", DB, want_b, rdb)):
                    if asked:
                        arena.check_guard(tag)
                        pairs[name] = (arena.packed()[0], r)
                    else:
                        arena.check_unchanged(tag + f" {name} (not asked for)")
                bwd_err("mcr_layernorm_backward", tag, pairs)
                if not acc and want_g and want_b:
                    if lay == "packed":
                        packed = pairs
                    elif lay == "pad4":
                        for k in pairs:
                            assert np.array_equal(pairs[k][0].view(np.int32), packed[k][0].view(np.int32)), f"{tag} {k}: differs from the packed call"
    X, DX, ws = Arena(8, E, data=x[:8] if M >= 8 else np.zeros((8, E), np.float32), device=dev), Arena(8, E, device=dev), Workspace(ws_bytes, dev)
    for ldx, ldy, ldd in ((E - 1, E, E), (E, E - 1, E), (E, E, E - 1)):
        rc = L_().mcr_layernorm_backward(P(X), I64(ldx), P(GM), P(X), I64(ldy), I64(8), CI(E), P(DX), I64(ldd), CI(0), VP(None), VP(None), P(ws),
                                         SZ(ws.n_bytes), stream())
        refused(rc, f"mcr_layernorm_backward ld {ldx, ldy, ldd}", "leading dimension too small", [DX, ws])


# =====================================================================================================================================
# mcr_colmax_backward
# =====================================================================================================================================
CB_LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0), "pad4": (4, 4, 4, 0, 0, 0), "odd": (1, 1, 1, 0, 0, 0), "offsets": (0, 0, 0, 1, 1, 1),
              "all": (1, 4, 1, 1, 0, 1)}


@pytest.mark.parametrize("E", [1, 63, 126, 256])
@pytest.mark.parametrize("L", [1, 17, 300, 2048])
def test_colmax_backward(dev, L, E):
    S = 3
    rng = np.random.default_rng(L * 7 + E)
    x = rng.standard_normal((S, L, E)).astype(np.float32)
    if L > 1:                                     # ties: the lowest valid row must win
        x[0, L - 1, 0] = x[0, L // 2, 0] = 10.0
        x[1, 1, E - 1] = x[1, 0, E - 1] = 9.0
        x[2, :, E // 2] = 1.0                     # a whole column tied: row 0
    g = rng.standard_normal((S, L, E)).astype(np.float32)
    base = rng.standard_normal((S, L, E)).astype(np.float32)
    for lens in (None, [L] * S, [1] * S, [L, max(1, L // 2), 1]):
        ref = st.colmax_backward_ref(x, g, lens) + base
        lt = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
        packed = None
        for lay, (px, pg, pd, ox, og, od) in CB_LAYOUTS.items():
            tag = f"L={L} E={E} lens={lens} {lay}"
            X, G = Arena(S * L, E, E + px, ox, x.reshape(-1, E), dev), Arena(S * L, E, E + pg, og, g.reshape(-1, E), dev)
            DX = Arena(S * L, E, E + pd, od, base.reshape(-1, E), dev)
            rc = L_().mcr_colmax_backward(P(X), I64(X.ld), P(G), I64(G.ld), P(DX), I64(DX.ld), I64(S), I64(L), CI(E),
                                          VP(lt.data_ptr() if lt is not None else None), stream())
            sync_ok(rc, tag)
            X.check_unchanged(tag)
            G.check_unchanged(tag)
            DX.check_guard(tag)
            d = DX.packed().reshape(S, L, E)
            bwd_err("mcr_colmax_backward", tag, {"dx": (d, ref)})
            touched = (d.view(np.int32) != base.view(np.int32)).sum(1)
            assert (touched <= 1).all(), f"{tag}: more than one row of a column received gradient"
            if lay == "packed":
                packed = d
            else:                                 # a fixed-order sum: the same bits wherever the rows lie
                assert np.array_equal(d.view(np.int32), packed.view(np.int32)), tag
    if E > 1:
        X, DX = Arena(S * L, E, data=x.reshape(-1, E), device=dev), Arena(S * L, E, device=dev)
        for ldx, ldg, ldd in ((E - 1, E, E), (E, E - 1, E), (E, E, E - 1)):
            rc = L_().mcr_colmax_backward(P(X), I64(ldx), P(X), I64(ldg), P(DX), I64(ldd), I64(S), I64(L), CI(E), VP(None), stream())
            refused(rc, f"mcr_colmax_backward ld {ldx, ldg, ldd}", "leading dimension too small", [DX])


# =====================================================================================================================================
# The network entry points in a workspace of exactly the size they ask for
# =====================================================================================================================================
# entry -> (its size function, the positions of that function's arguments among the entry's, the position of `workspace` (the byte
# count follows it), the position of `phase` or None, outputs: position -> (rows, cols) from the arguments)
def _vis_rows(a):
    return a[3].value * a[4].value


NET_ENTRIES = {
    "mcr_pc_transformer_forward": ("mcr_pc_transformer_workspace_bytes", (2, 3), 7, None, lambda a: {1: (a[2].value, a[4].value)}),
    "mcr_scone_vis_forward": ("mcr_scone_vis_workspace_bytes", (3, 4), 8, None, lambda a: {2: (_vis_rows(a), 64)}),
    "mcr_scone_vis_backward": ("mcr_scone_vis_backward_workspace_bytes", (3, 4), 11, None, lambda a: {9: (_vis_rows(a), 4), 10: (_vis_rows(a), 64)}),
    "mcr_scone_occ_forward_phase": ("mcr_scone_occ_workspace_bytes", (7, 8, 1), 15, 17, lambda a: {6: (a[7].value * a[8].value, 1)}),
    "mcr_scone_occ_forward_ragged_phase": ("mcr_scone_occ_ragged_workspace_bytes", (11, 12, 2), 19, 21, lambda a: {10: (a[12].value, 1)}),
}
VIS_D_WEIGHTS = 8                                      # mcr_scone_vis_backward: the table of 48 gradient pointers
_ENC_SHAPES = [(1, 256), (1, 256), (384, 256), (1, 384), (256, 256), (1, 256), (1, 256), (1, 256), (512, 256), (1, 512), (256, 512), (1, 256)]
VIS_TABLE_SHAPES = [(126, 4), (1, 126), (126, 126), (1, 126)] + 3 * _ENC_SHAPES + \
                   [(1, 256), (1, 256), (192, 256), (1, 192), (128, 256), (1, 128), (64, 128), (1, 64)]       # include/macarons_hip.h: SCONE_VIS (48)


def _is_null(p):
    return p is None or getattr(p, "value", 1) in (None, 0)


class ExactWorkspaces:
    """Stands in front of the network entry points of the loaded library.  Every call that reaches one of them (through ops.*, with the
    operands ops.* made) goes through unchanged and is then REPEATED through ctypes, same operands, same variant, with
      - a workspace of exactly the bytes the entry's size function returns, inside a guarded, NaN-filled arena, and outputs in
        guarded arenas of their own: return code 0, guards intact; the outputs are kept (`calls`) for the bit comparison with
        what ops.* returned;
      - a workspace 4 bytes shorter: the entry must refuse (code 1, "workspace too small", outputs untouched).
    The two calls of a two-phase forward share one exact workspace, as the header asks."""

    def __init__(self, monkeypatch, dev):
        from macarons_amd import ops
        self.ops, self.dev, self.lib = ops, dev, L_()
        self.real = {name: getattr(self.lib, name) for name in NET_ENTRIES}
        self.kept = {}                                 # entry -> the exact workspace of its current forward
        self.calls = []                                # (entry, phase, {position: packed output})
        for name in NET_ENTRIES:
            monkeypatch.setattr(self.lib, name, lambda *a, _n=name: self._call(_n, a), raising=False)

    def _repeat(self, name, args, ws, outs):
        a = list(args)
        wpos = NET_ENTRIES[name][2]
        a[wpos], a[wpos + 1] = P(ws), SZ(ws.n_bytes)
        for pos, arena in outs.items():
            a[pos] = (VP * len(arena))(*[x.ptr for x in arena]) if isinstance(arena, list) else P(arena)
        self.lib.mcr_call_variant(CI(getattr(self.ops._tls, "variant", 0)))
        rc = self.real[name](*a)
        torch.cuda.synchronize()
        return rc

    def _outs(self, name, args):
        outs = {pos: Arena(r, c, device=self.dev) for pos, (r, c) in NET_ENTRIES[name][4](args).items() if not _is_null(args[pos])}
        if name == "mcr_scone_vis_backward" and not _is_null(args[VIS_D_WEIGHTS]):
            outs[VIS_D_WEIGHTS] = [Arena(r, c, device=self.dev) for r, c in VIS_TABLE_SHAPES]
        return outs

    def _call(self, name, args):
        rc = self.real[name](*args)
        if rc != 0:
            return rc
        size_fn, size_pos, wpos, ppos, _ = NET_ENTRIES[name]
        phase = args[ppos].value if ppos is not None else 0
        tag = f"{name} phase {phase} variant {self.ops.current_variant()} sizes {[args[i].value for i in size_pos]}"
        n = int(getattr(self.lib, size_fn)(*[args[i] for i in size_pos]))
        if phase != 2:
            self.kept[name] = Workspace(n, self.dev)
        ws = self.kept[name]
        assert ws.n_bytes == n, f"{tag}: phase 2 asks for {n} bytes, phase 1 asked for {ws.n_bytes}"
        outs = self._outs(name, args)
        rc2 = self._repeat(name, args, ws, outs)
        assert rc2 == 0, f"{tag}: rc {rc2} in a workspace of exactly {n} bytes: {last_error()}"
        ws.check_guard(tag + " workspace")
        flat = [x for v in outs.values() for x in (v if isinstance(v, list) else [v])]
        for x in flat:
            x.check_guard(tag + " output")
        self.calls.append((name, phase, {pos: ([x.packed() for x in v] if isinstance(v, list) else v.packed()) for pos, v in outs.items()}))
        short, outs = Workspace(n - 4, self.dev), self._outs(name, args)
        rc3 = self._repeat(name, args, short, outs)
        refused(rc3, tag + f" in {n - 4} bytes", "workspace too small", [short] + [x for v in outs.values() for x in (v if isinstance(v, list) else [v])])
        assert rc3 == 1, f"{tag}: a short workspace returned {rc3}"
        print(f"EXACT {tag}: {n} bytes")
        return rc

    def take(self, name, phase=None):
        """The kept outputs of the calls of `name` since the last take (those of `phase` only, if given)."""
        got = [o for (n_, ph, o) in self.calls if n_ == name and (phase is None or ph == phase)]
        self.calls = []
        return got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and np.array_equal(a.reshape(-1).view(np.int32), b.reshape(-1).view(np.int32))


def _golden_module(cls, seed, dev):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import weights
    m = cls()
    sd = weights.make_state_dict(weights.shapes_of(m), seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def _to(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


NET_VARIANTS = [1, 5, 6, 7]


@pytest.mark.parametrize("variant", NET_VARIANTS)
def test_exact_workspace_pc_transformer_and_scone_occ(dev, monkeypatch, variant):
    """mcr_pc_transformer_forward, mcr_scone_occ_forward (single call; phases 1 + 2; a batch of clouds; the layer-by-layer path) on the
    golden weights and sizes, each in a workspace of exactly its stated size (ExactWorkspaces)."""
    from conftest import golden
    from macarons_amd import ops
    from macarons_amd.networks import SconeOcc
    m = _golden_module(SconeOcc, 2, dev)
    g = golden("scone_occ")
    spy = ExactWorkspaces(monkeypatch, dev)
    with torch.no_grad(), ops.variant(variant):
        for tag in ("m100_q17", "m1024_q300", "m4096_q512"):
            perms = [torch.from_numpy(g[f"{tag}_perm{i}"].astype(np.int64)) for i in range(3)]
            pc, x, vh = _to(g[f"{tag}_pc"], dev), _to(g[f"{tag}_x"], dev), _to(g[f"{tag}_vh"], dev)
            gf = m.global_transformer(pc[:, perms[0].to(dev)].contiguous()).cpu().numpy()
            (o,) = spy.take("mcr_pc_transformer_forward")
            assert same_bits(o[1], gf), f"{tag}: mcr_pc_transformer_forward in an exact workspace differs from ops.pc_transformer_forward"
            y = m(pc, x, vh, perms=perms).cpu().numpy()
            (o,) = spy.take("mcr_scone_occ_forward_phase", 0)
            assert same_bits(o[6], y), f"{tag}: single call"
            if min(m.scale_sizes(pc.shape[1])) < m.k_for_knn:        # (m100: its coarsest cloud is below k, forward_begin does not apply)
                continue
            h = m.forward_begin(pc, x)
            assert h is not None
            y2 = m(pc, x, vh, perms=perms, begun=h).cpu().numpy()
            got = spy.take("mcr_scone_occ_forward_phase")
            assert len(got) == 2 and not got[0] and same_bits(got[1][6], y2) and same_bits(y2, y), f"{tag}: phases 1 + 2"
        # a batch of clouds (one search and one transformer launch per scale over all rows), Q beyond one chunk of the layer-by-layer path
        rng = np.random.default_rng(5)
        pc = _to(rng.uniform(-.4, .4, (2, 1500, 3)).astype(np.float32), dev)
        x = _to(rng.uniform(-.5, .5, (2, 16385, 3)).astype(np.float32), dev)
        vh = _to((rng.standard_normal((2, 16385, 64)) * .3).astype(np.float32), dev)
        torch.manual_seed(5)
        perms = m.draw_perms(1500)
        y = m(pc, x, vh, perms=perms).cpu().numpy()
        (o,) = spy.take("mcr_scone_occ_forward_phase", 0)
        assert same_bits(o[6], y), "batch of two clouds"
        m.fused_local = False
        y = m(pc, x, vh, perms=perms).cpu().numpy()
        (o,) = spy.take("mcr_scone_occ_forward_phase", 0)
        assert same_bits(o[6], y), "layer-by-layer path"


@pytest.mark.parametrize("variant", NET_VARIANTS)
def test_exact_workspace_scone_occ_ragged(dev, monkeypatch, variant):
    """mcr_scone_occ_forward_ragged: phases 1 + 2 (SconeOcc.forward_ragged), then the single call on the operands of that phase 2."""
    from macarons_amd import ops
    from macarons_amd.networks import SconeOcc
    m = _golden_module(SconeOcc, 2, dev)
    rng = np.random.default_rng(12)
    sizes_m, sizes_q = [100, 3000, 65, 2048, 900], [17, 300, 1, 129, 4097]
    pc = _to(np.concatenate([rng.uniform(-.4, .4, (n, 3)).astype(np.float32) for n in sizes_m]), dev)
    x = _to(np.concatenate([rng.uniform(-.5, .5, (q, 3)).astype(np.float32) for q in sizes_q]), dev)
    vh = _to(np.concatenate([(rng.standard_normal((q, 64)) * .3).astype(np.float32) for q in sizes_q]), dev)
    torch.manual_seed(21)
    perms = [m.draw_perms(n) for n in sizes_m]
    spy = ExactWorkspaces(monkeypatch, dev)
    real, last = ops.scone_occ_forward_ragged, {}

    def keep(*a, **k):                                  # the operands the module made for its last call (they stay alive here)
        last["a"], last["k"] = a, k
        return real(*a, **k)
    monkeypatch.setattr(ops, "scone_occ_forward_ragged", keep)
    with torch.no_grad(), ops.variant(variant):
        y = m.forward_ragged(pc, sizes_m, x, vh, sizes_q, perms=perms).cpu().numpy()
        got = spy.take("mcr_scone_occ_forward_ragged_phase")
        assert [len(o) for o in got] == [0, 1] and same_bits(got[1][10], y), "phases 1 + 2"
        assert last["k"]["phase"] == 2
        y0 = real(*last["a"], **{**last["k"], "phase": 0, "out": None}).cpu().numpy()
        (o,) = spy.take("mcr_scone_occ_forward_ragged_phase", 0)
        assert same_bits(o[10], y0) and same_bits(y0, y), "single call"


@pytest.mark.parametrize("variant", NET_VARIANTS)
def test_exact_workspace_scone_vis_forward(dev, monkeypatch, variant):
    from conftest import golden
    from macarons_amd import ops
    from macarons_amd.networks import SconeVis
    m = _golden_module(SconeVis, 1, dev)
    g = golden("scone_vis")
    spy = ExactWorkspaces(monkeypatch, dev)
    with torch.no_grad(), ops.variant(variant):
        for key in ("16", "333", "2048", "b3"):
            y = m(_to(g[f"pts_{key}"], dev), view_harmonics=_to(g[f"vh_{key}"], dev)).cpu().numpy()
            (o,) = spy.take("mcr_scone_vis_forward")
            assert same_bits(o[2], y), key
        lengths = torch.tensor([700, 2048, 1], dtype=torch.int32, device=dev)
        pts, vh = _to(np.tile(g["pts_2048"], (3, 1, 1)), dev), _to(np.tile(g["vh_2048"], (3, 1, 1)), dev)
        y = m(pts, view_harmonics=vh, lengths=lengths).cpu().numpy()
        (o,) = spy.take("mcr_scone_vis_forward")
        assert same_bits(o[2], y), "padded batch with lengths"


@pytest.mark.parametrize("B,N,with_lengths", [(1, 333, False), (1, 2048, False), (3, 700, True)])
def test_exact_workspace_scone_vis_backward(dev, monkeypatch, B, N, with_lengths):
    """mcr_scone_vis_backward takes no variant (the fp32 network's gradient on every one): all three gradients, then each alone."""
    from macarons_amd import ops
    from macarons_amd.networks import SconeVis
    m = _golden_module(SconeVis, 1, dev)
    rng = np.random.default_rng(B * N)
    pts = _to(rng.uniform(-.5, .5, (B, N, 4)).astype(np.float32), dev)
    vh = _to((rng.standard_normal((B, N, 64)) * .3).astype(np.float32), dev)
    d_out = _to(rng.standard_normal((B, N, 64)).astype(np.float32), dev)
    lengths = torch.tensor([N, N // 2, 1][:B], dtype=torch.int32, device=dev) if with_lengths else None
    spy = ExactWorkspaces(monkeypatch, dev)
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        d_w, d_pts, d_vh = ops.scone_vis_backward(pts, vh, d_out, m.weight_table(), lengths, need=need)
        (o,) = spy.take("mcr_scone_vis_backward")
        assert set(o) == {p for p, asked in zip((VIS_D_WEIGHTS, 9, 10), need) if asked}, need
        if need[0]:
            for i, (got, ref) in enumerate(zip(o[VIS_D_WEIGHTS], d_w)):
                assert same_bits(got, ref.cpu().numpy()), f"need {need}: d_weights[{i}]"
        if need[1]:
            assert same_bits(o[9], d_pts.cpu().numpy()), f"need {need}: d_pts"
        if need[2]:
            assert same_bits(o[10], d_vh.cpu().numpy()), f"need {need}: d_view_harmonics"
