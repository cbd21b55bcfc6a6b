"""The PCTransformer backward's C ABI (include/macarons_hip.h: mcr_attention_backward_pct, mcr_pool_max_avg_backward,
mcr_pc_transformer_backward) on the arenas of tests/_strided.py: padded leading dimensions, the guard fill intact after the call,
workspaces of exactly *_workspace_bytes, and refusals (misaligned operand, short workspace, lens with 16-token sequences, more than
65 535 longer sequences) that return non-zero and write nothing.  BLOCK_TOL = 2e-5 on max |got - ref| / max |ref| per tensor against
the fp64 references of _strided.py; the network entry must give the bits of the call through ops.*.  Errors are printed with ERR."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _strided as st
from _strided import Arena, Workspace

pytestmark = pytest.mark.gpu

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


def bwd_err(entry, tag, pairs):
    es = {k: st.rel_max(g, r) for k, (g, r) in pairs.items()}
    print(f"ERR {entry} {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in es.items()))
    for k, (g, _) in pairs.items():
        assert np.isfinite(g).all(), f"{entry} {tag}: non-finite {k}"
    assert max(es.values()) < BLOCK_TOL, f"{entry} {tag}: {es}"


def refused(rc, what, needle, outs):
    torch.cuda.synchronize()
    for o in outs:
        o.check_unchanged(f"{what}: output of a refused call")
    assert rc != 0, f"{what}: the call must be refused; it returned 0 (message buffer: {last_error()!r})"
    assert needle in last_error(), f"{what}: message {last_error()!r} lacks {needle!r}"
    print(f"REFUSED {what}")


# ---- mcr_attention_backward_pct -------------------------------------------------------------------------------------------------------
def _ab_call(Q, G, D, S, L, lt, ws, lds=None):
    ldq, ldg, ldd = lds or (Q.ld, G.ld, D.ld)
    return L_().mcr_attention_backward_pct(P(Q), I64(ldq), P(G), I64(ldg), P(D), I64(ldd), I64(S), I64(L), CI(4), CI(32), CI(128),
                                           VP(lt.data_ptr() if lt is not None else None), P(ws), SZ(ws.n_bytes if ws is not None else 0),
                                           stream())


def _ab_ref(qkv, g, lens):
    return np.concatenate([st.attention_backward_ref(qkv[s:s + 1], g[s:s + 1], 4, 32, 128, None if lens is None else lens[s:s + 1])
                           for s in range(qkv.shape[0])])


@pytest.mark.parametrize("S,L,with_lens", [(5, 16, False), (1031, 16, False), (2, 17, True), (3, 333, False), (3, 333, True)])
def test_attention_backward_pct(dev, S, L, with_lens):
    rng = np.random.default_rng(S * 1000 + L)
    qkv = rng.standard_normal((S, L, 192)).astype(np.float32)
    g = rng.standard_normal((S, L, 128)).astype(np.float32)
    lens = np.array([1] + [max(1, L // 2 - 3)] * (S - 1), np.int32) if with_lens else None
    lt = torch.from_numpy(lens).to(dev) if with_lens else None
    ref = _ab_ref(qkv, g, lens)
    nb = int(L_().mcr_attention_backward_pct_workspace_bytes(I64(S), I64(L)))
    packed = None
    for pads in [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 8, 12)]:
        tag = f"S={S} L={L} lens={with_lens} ld+{pads}"
        Q = Arena(S * L, 192, 192 + pads[0], 0, qkv.reshape(-1, 192), dev)
        G = Arena(S * L, 128, 128 + pads[1], 0, g.reshape(-1, 128), dev)
        D = Arena(S * L, 192, 192 + pads[2], 0, device=dev)
        ws = Workspace(nb, dev)
        sync_ok(_ab_call(Q, G, D, S, L, lt, ws), tag)
        D.check_guard(tag)
        ws.check_guard(tag + " workspace")
        if L == 16:
            ws.check_unchanged(tag + ": the 16-token kernel touches no workspace")
        Q.check_unchanged(tag)
        G.check_unchanged(tag)
        d = D.packed().reshape(S, L, 192)
        bwd_err("mcr_attention_backward_pct", tag, {"dq": (d[..., :32], ref[..., :32]), "dk": (d[..., 32:64], ref[..., 32:64]),
                                                     "dv": (d[..., 64:], ref[..., 64:])})
        if with_lens:
            for s in range(S):
                assert not d[s, int(lens[s]):, 32:].any(), tag
        if packed is None:
            packed = d
        else:
            assert np.array_equal(d.view(np.int32), packed.view(np.int32)), f"{tag}: differs from the packed call"


def test_attention_backward_pct_refusals(dev):
    rng = np.random.default_rng(0)
    who = "mcr_attention_backward_pct"
    for S, L in ((2, 17), (3, 16)):
        qkv, g = rng.standard_normal((S * L, 192)).astype(np.float32), rng.standard_normal((S * L, 128)).astype(np.float32)
        nb = int(L_().mcr_attention_backward_pct_workspace_bytes(I64(S), I64(L)))
        mk = lambda pq=0, pg=0, pd=0, oq=0, og=0, od=0, ow=0, short=0: (
            Arena(S * L, 192, 192 + pq, oq, qkv, dev), Arena(S * L, 128, 128 + pg, og, g, dev), Arena(S * L, 192, 192 + pd, od, device=dev),
            Workspace(nb - short, dev, offset=ow))
        cases = [({"pq": 1}, "multiples of 4"), ({"pg": 1}, "multiples of 4"), ({"pd": 1}, "multiples of 4"),
                 ({"oq": 1}, "16-byte aligned"), ({"og": 1}, "16-byte aligned"), ({"od": 1}, "16-byte aligned")]
        if L != 16:                                 # (the 16-token path takes no workspace)
            cases += [({"ow": 1}, "workspace must be 16-byte aligned"), ({"short": 4}, "workspace too small")]
        for kw, needle in cases:
            Q, G, D, ws = mk(**kw)
            refused(_ab_call(Q, G, D, S, L, None, ws), f"{who} L={L} {kw}", needle, [D, ws])
        Q, G, D, ws = mk()
        for lds in ((188, 128, 192), (192, 124, 192), (192, 128, 188)):
            refused(_ab_call(Q, G, D, S, L, None, ws, lds), f"{who} L={L} ld {lds}", "leading dimensions must cover the rows", [D, ws])
        if L == 16:
            lt = torch.full((S,), 9, dtype=torch.int32, device=dev)
            refused(_ab_call(Q, G, D, S, L, lt, ws), f"{who} lens with L = 16", "take no lens", [D, ws])
    # more than 65 535 sequences of another length than 16: refused on the host before anything is read (the operands are full size)
    S, L = 65536, 17
    Q, G, D = Arena(S * L, 192, device=dev), Arena(S * L, 128, device=dev), Arena(S * L, 192, device=dev)
    ws = Workspace(1024, dev)
    refused(_ab_call(Q, G, D, S, L, None, ws), f"{who} S={S} L={L}", "bad problem size", [D, ws])


# ---- mcr_pool_max_avg_backward --------------------------------------------------------------------------------------------------------
def _pool_ref(x, g):
    S, L, E = x.shape
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    (torch.cat((xd.max(dim=1)[0], xd.mean(dim=1)), dim=-1) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return xd.grad.numpy()


@pytest.mark.parametrize("S,L,E", [(7, 16, 128), (3, 150, 256), (1, 2048, 256), (2, 33, 100)])
def test_pool_max_avg_backward(dev, S, L, E):
    rng = np.random.default_rng(S + L + E)
    x = rng.standard_normal((S, L, E)).astype(np.float32)
    g = rng.standard_normal((S, 2 * E)).astype(np.float32)
    ref = _pool_ref(x, g)
    # (ldx - E, ldy - 2E, ld_dx - E, offsets X, dY, dX): scalar accesses, any leading dimension and 4-byte alignment
    for lay in [(0, 0, 0, 0, 0, 0), (4, 4, 4, 0, 0, 0), (1, 3, 5, 0, 0, 0), (0, 0, 0, 1, 2, 3), (1, 3, 4, 1, 1, 1)]:
        tag = f"S={S} L={L} E={E} layout {lay}"
        X = Arena(S * L, E, E + lay[0], lay[3], x.reshape(-1, E), dev)
        Y = Arena(S, 2 * E, 2 * E + lay[1], lay[4], g, dev)
        D = Arena(S * L, E, E + lay[2], lay[5], device=dev)
        sync_ok(L_().mcr_pool_max_avg_backward(P(X), I64(X.ld), P(Y), I64(Y.ld), P(D), I64(D.ld), I64(S), I64(L), CI(E), stream()), tag)
        D.check_guard(tag)
        X.check_unchanged(tag)
        Y.check_unchanged(tag)
        bwd_err("mcr_pool_max_avg_backward", tag, {"dx": (D.packed().reshape(S, L, E), ref)})
    X, Y, D = Arena(S * L, E, data=x.reshape(-1, E), device=dev), Arena(S, 2 * E, data=g, device=dev), Arena(S * L, E, device=dev)
    for lds in ((E - 1, 2 * E, E), (E, 2 * E - 1, E), (E, 2 * E, E - 1)):
        refused(L_().mcr_pool_max_avg_backward(P(X), I64(lds[0]), P(Y), I64(lds[1]), P(D), I64(lds[2]), I64(S), I64(L), CI(E), stream()),
                f"mcr_pool_max_avg_backward ld {lds}", "leading dimension too small", [D])


# ---- mcr_pc_transformer_backward -----------------------------------------------------------------------------------------------------
def _pct(dev, L, feature_dim):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import weights
    from macarons_amd.networks.SconeOcc import PCTransformer
    m = PCTransformer(seq_len=L, pts_embedding_dim=128, feature_dim=feature_dim)
    sd = weights.make_state_dict(weights.shapes_of(m), 12)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def _pb_call(pc, g, S, L, fd, tab, dw, dpc, ws, n_bytes=None):
    wtab = (VP * len(tab))(*[t.data_ptr() for t in tab])
    dtab = (VP * len(dw))(*[a.ptr for a in dw]) if dw is not None else VP(None)
    return L_().mcr_pc_transformer_backward(P(pc), P(g), I64(S), I64(L), CI(fd), wtab, CI(len(tab)), dtab, P(dpc), P(ws),
                                            SZ(ws.n_bytes if n_bytes is None else n_bytes), stream())


@pytest.mark.parametrize("S,L,fd", [(5, 16, 256), (2, 150, 512), (1, 600, 512)])
def test_pc_transformer_backward_exact_workspace(dev, S, L, fd):
    """All gradients, then each alone, in a workspace of exactly the stated size with guarded outputs: the bits of ops.*; 4 bytes less,
    a misaligned operand and too many long sequences are refused."""
    from macarons_amd import ops
    m = _pct(dev, L, fd)
    tab = m.weight_table_with_planes() if L >= 512 else m.weight_table()        # (a PLANES / END PLANES tail is accepted and ignored)
    rng = np.random.default_rng(S * L)
    pc = rng.uniform(-.4, .4, (S * L, 3)).astype(np.float32)
    g = rng.standard_normal((S, fd)).astype(np.float32)
    pct, gt = torch.from_numpy(pc).to(dev).view(S, L, 3), torch.from_numpy(g).to(dev)
    nb = int(L_().mcr_pc_transformer_backward_workspace_bytes(I64(S), I64(L)))
    shapes = [tuple(t.reshape(-1, t.shape[-1]).shape) if t.dim() == 2 else (1, t.numel()) for t in tab[:32]]
    mk = lambda: (Arena(S * L, 3, data=pc, device=dev), Arena(S, fd, data=g, device=dev), [Arena(r, c, device=dev) for r, c in shapes],
                  Arena(S * L, 3, device=dev))
    for need in ((True, True), (True, False), (False, True)):
        tag = f"S={S} L={L} need {need}"
        d_w, d_pc = ops.pc_transformer_backward(pct, gt, tab, fd, need=need)
        PC, GF, DW, DP = mk()
        ws = Workspace(nb, dev)
        sync_ok(_pb_call(PC, GF, S, L, fd, tab, DW if need[0] else None, DP if need[1] else None, ws), tag)
        ws.check_guard(tag + " workspace")
        PC.check_unchanged(tag)
        GF.check_unchanged(tag)
        for i, a in enumerate(DW):
            if need[0]:
                a.check_guard(f"{tag} d_weights[{i}]")
                assert np.array_equal(a.packed().reshape(-1).view(np.int32), d_w[i].cpu().numpy().reshape(-1).view(np.int32)), f"{tag}: d_weights[{i}]"
            else:
                a.check_unchanged(f"{tag} d_weights[{i}]")
        if need[1]:
            DP.check_guard(tag + " d_pc")
            assert np.array_equal(DP.packed().reshape(-1).view(np.int32), d_pc.cpu().numpy().reshape(-1).view(np.int32)), f"{tag}: d_pc"
        else:
            DP.check_unchanged(tag + " d_pc")
    who = "mcr_pc_transformer_backward"
    PC, GF, DW, DP = mk()
    short = Workspace(nb - 4, dev)
    refused(_pb_call(PC, GF, S, L, fd, tab, DW, DP, short), f"{who} in {nb - 4} bytes", "workspace too small", [short, DP] + DW)
    ws = Workspace(nb, dev)
    PC1 = Arena(S * L, 3, offset=1, data=pc, device=dev)
    refused(_pb_call(PC1, GF, S, L, fd, tab, DW, DP, ws), f"{who} pc off the 16-byte grid", "16-byte aligned", [ws, DP] + DW)
    ws1 = Workspace(nb, dev, offset=1)
    refused(_pb_call(PC, GF, S, L, fd, tab, DW, DP, ws1, nb + 64), f"{who} workspace off the 16-byte grid", "16-byte aligned", [ws1, DP] + DW)
    if L != 16:                                     # refused on the size alone, before anything is read
        refused(_pb_call(PC, GF, 65536, L, fd, tab, DW, DP, ws, 1 << 62), f"{who} S=65536 L={L}", "bad problem size", [ws, DP] + DW)
    sync_ok(_pb_call(PC, GF, S, L, fd, tab, None, None, ws), "both NULL")           # nothing asked: returns 0 at once
    ws.check_unchanged("both NULL")
