"""Arenas for calling the C ABI (include/macarons_hip.h) on strided, offset and guarded operands, and the fp64 references of the
building blocks.  TEST INFRASTRUCTURE ONLY.

An Arena is ONE allocation that is larger than its operand on every side:

    [ LEAD floats | offset floats | row 0: cols values, ld - cols padding | row 1 ... | row rows-1 (padding included) | GUARD floats ]

The buffer starts 256-byte aligned; the operand starts LEAD + offset floats into it (offset 0..3 moves it off the 16-byte grid).
Everything outside the logical [rows, cols] window holds FILL, a quiet NaN with a fixed payload that no kernel produces, and is
compared as int32: check_guard() names every element outside the window whose bits changed (the floats before the first row, the
padding columns cols .. ld-1 of every row, the GUARD floats behind the last row).  The guard is inside the same allocation on
purpose: an overrun of a few rows lands in our own memory and is reported, it does not leave the allocation.  check_unchanged()
compares the whole buffer with its state at creation: inputs, and outputs of calls that were refused.

HalfArena is the same layout for fp16 operands (the hi / lo planes of the planes GEMMs), every quantity counted in halves.  Its fill
is a half-precision NaN with a fixed payload in EVERY half (FILL_BITS seen as two halves is a NaN and -1.73): a guard half that
reaches an accumulator poisons the output.
"""
import numpy as np
import torch

FILL_BITS = 0x7FC0BEEF           # quiet NaN, payload 0xBEEF
GUARD = 4096                     # floats behind the last row
LEAD = 64                        # floats (256 bytes) before the operand
HALF_FILL_BITS = 0x7EEF          # fp16 quiet NaN, payload 0xEF
HALF_GUARD = 2 * GUARD           # halves behind the last row (the same bytes)
HALF_LEAD = 2 * LEAD             # halves (256 bytes) before the operand


class Arena:
    # element type of the operand, the integer type its bits are compared as, and the layout constants in elements
    T_VAL, T_BITS, NP_VAL, NP_BITS, ITEM = torch.float32, torch.int32, np.float32, np.int32, 4
    FILL, LEAD_N, GUARD_N = FILL_BITS, LEAD, GUARD

    def __init__(self, rows, cols, ld=None, offset=0, data=None, device="cpu", guard=None):
        ld = cols if ld is None else ld
        guard = self.GUARD_N if guard is None else guard
        assert rows > 0 and cols > 0 and ld >= cols and 0 <= offset < self.LEAD_N and guard >= self.GUARD_N
        self.rows, self.cols, self.ld, self.offset, self.guard = rows, cols, ld, offset, guard
        self.start = self.LEAD_N + offset
        self.n = self.start + rows * ld + guard
        self.bits = torch.full((self.n,), self.FILL, dtype=self.T_BITS, device=device)
        assert not self.bits.is_cuda or self.bits.data_ptr() % 256 == 0
        self.floats = self.bits.view(self.T_VAL)
        if data is not None:
            d = torch.as_tensor(np.ascontiguousarray(data, dtype=self.NP_VAL) if isinstance(data, np.ndarray) else data)
            assert tuple(d.shape) == (rows, cols) and d.dtype == self.T_VAL, (d.shape, d.dtype)
            self.window().copy_(d)
        self.initial = self.bits.clone()

    @property
    def ptr(self):
        """Device address of element (0, 0) of the operand."""
        return self.bits.data_ptr() + self.ITEM * self.start

    def window(self):
        """The logical [rows, cols] matrix as a strided view of the arena."""
        return self.floats.as_strided((self.rows, self.cols), (self.ld, 1), self.start)

    def packed(self):
        """A packed host copy of the logical matrix (numpy, the arena's element type)."""
        return self.window().cpu().contiguous().numpy()

    def outside_mask(self):
        m = np.ones(self.n, dtype=bool)
        body = m[self.start:self.start + self.rows * self.ld].reshape(self.rows, self.ld)
        body[:, :self.cols] = False
        return m

    def region(self, i):
        if i < self.start:
            return "before the first row"
        if i >= self.start + self.rows * self.ld:
            return f"guard +{i - self.start - self.rows * self.ld}"
        r, c = divmod(i - self.start, self.ld)
        return f"padding row {r} col {c}"

    def guard_violations(self):
        bits = self.bits.cpu().numpy()
        bad = np.flatnonzero(self.outside_mask() & (bits != self.NP_BITS(self.FILL)))
        return [(int(i), self.region(int(i))) for i in bad]

    def check_guard(self, what=""):
        bad = self.guard_violations()
        assert not bad, f"{what}: {len(bad)} stray write(s) outside the [{self.rows}, {self.cols}] window (ld {self.ld}): {bad[:8]}"

    def check_unchanged(self, what=""):
        diff = torch.nonzero(self.bits != self.initial).flatten().cpu().numpy()
        assert diff.size == 0, f"{what}: {diff.size} element(s) changed, first at {[(int(i), self.region(int(i))) for i in diff[:8]]}"


class HalfArena(Arena):
    """An arena of fp16 values: rows, cols, ld, offset and the guard are counted in halves (offset 0..7 moves the operand off the
    16-byte grid); `floats` holds halves, packed() returns float16, packed_bits() the same as uint16."""
    T_VAL, T_BITS, NP_VAL, NP_BITS, ITEM = torch.float16, torch.int16, np.float16, np.int16, 2
    FILL, LEAD_N, GUARD_N = HALF_FILL_BITS, HALF_LEAD, HALF_GUARD

    def packed_bits(self):
        return self.packed().view(np.uint16)


class Workspace(Arena):
    """Exactly n_bytes of scratch (a multiple of 4; 256-byte aligned unless offset) inside a larger arena: its interior starts as
    FILL (a kernel reading scratch it never wrote computes NaNs), the bytes before and behind it are checked like any guard."""

    def __init__(self, n_bytes, device="cpu", offset=0):
        assert n_bytes % 4 == 0
        self.n_bytes = n_bytes
        super().__init__(1, max(1, n_bytes // 4), device=device, offset=offset)


# ---- fp64 references of the building blocks (numpy, or fp64 torch autograd, on the CPU) ---------------------------------------------
def gelu64(x):
    from math import sqrt
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x) / sqrt(2.0)).numpy())


def linear_ref(x, w, b=None, gelu=False, r=None):
    y = x.astype(np.float64) @ w.astype(np.float64).T
    if b is not None:
        y = y + b.astype(np.float64)
    if gelu:
        y = gelu64(y)
    if r is not None:
        y = y + r.astype(np.float64)
    return y


def layernorm_ref(x, g, b, eps=1e-5):
    x = x.astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g.astype(np.float64) + b.astype(np.float64)


def attention_ref(qkv, H, qk, v, mask=None, lens=None):
    """qkv [S, L, 2 qk + v] -> [S, L, v].  mask (optional, bool / 0-1, broadcastable to [S, H, L, L]): where it is 0 the score is
    replaced by -1e3 BEFORE the division by sqrt(d) (Attention.py:24-27).  lens (optional, [S]): keys = the first
    min(L, max(1, lens[s])) rows."""
    S, L, _ = qkv.shape
    x = qkv.astype(np.float64)
    hs = lambda t, d: t.reshape(S, L, H, d).transpose(0, 2, 1, 3)
    q, k, vv = hs(x[..., :qk], qk // H), hs(x[..., qk:2 * qk], qk // H), hs(x[..., 2 * qk:], v // H)
    sc = q @ k.transpose(0, 1, 3, 2)
    if mask is not None:
        sc = np.where(np.broadcast_to(np.asarray(mask).astype(bool), sc.shape), sc, -1e3)
    sc = sc / np.sqrt(qk // H)
    if lens is not None:
        n = np.clip(np.asarray(lens), 1, L).reshape(S, 1, 1, 1)
        sc = np.where(np.arange(L).reshape(1, 1, 1, L) < n, sc, -np.inf)
    sc = np.exp(sc - sc.max(-1, keepdims=True))
    return ((sc / sc.sum(-1, keepdims=True)) @ vv).transpose(0, 2, 1, 3).reshape(S, L, v)


def attention_backward_ref(qkv, g, H, qk, v, lens=None):
    """d (sum o * g) / d qkv in fp64 (torch autograd); qkv [S, L, 2 qk + v], g [S, L, v]."""
    S, L, _ = qkv.shape
    x = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    dq, dv = qk // H, v // H
    q = x[..., :qk].reshape(S, L, H, dq).transpose(1, 2)
    k = x[..., qk:2 * qk].reshape(S, L, H, dq).transpose(1, 2)
    vv = x[..., 2 * qk:].reshape(S, L, H, dv).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / np.sqrt(dq)
    if lens is not None:
        n = torch.from_numpy(np.clip(np.asarray(lens), 1, L).astype(np.int64)).view(-1, 1, 1, 1)
        s = s.masked_fill(torch.arange(L)[None, None, None, :] >= n, float("-inf"))
    o = (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(S, L, v)
    (o * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return x.grad.numpy()


def linear_backward_ref(x, w, b, g, gelu):
    """(dX, dW, db, Z) of sum(act(x w^T + b) * g) in fp64."""
    xd, wd, bd = (torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (x, w, b))
    z = torch.nn.functional.linear(xd, wd, bd)
    y = torch.nn.functional.gelu(z) if gelu else z
    (y * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return xd.grad.numpy(), wd.grad.numpy(), bd.grad.numpy(), z.detach().numpy()


def layernorm_backward_ref(x, gamma, g):
    E = x.shape[-1]
    xd, gd = (torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (x, gamma))
    bd = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.layer_norm(xd, (E,), gd, bd, 1e-5) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return xd.grad.numpy(), gd.grad.numpy(), bd.grad.numpy()


def colmax_backward_ref(x, g, lens=None):
    """x, g [S, L, E]: every column's summed gradient lands on the lowest valid row holding the column's max."""
    S, L, E = x.shape
    out = np.zeros((S, L, E), np.float64)
    tot = g.astype(np.float64).sum(1)
    for s in range(S):
        n = L if lens is None else int(min(L, max(1, lens[s])))
        arg = x[s, :n].argmax(0)                          # numpy: first occurrence = lowest row
        out[s, arg, np.arange(E)] = tot[s]
    return out


def rel_max(got, ref):
    """max |got - ref| / max |ref| (the backward tests' measure)."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
