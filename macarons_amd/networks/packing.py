"""Host-side packing of one local PCTransformer's parameters into the image local_pct.hip consumes.

Layout (must match macarons_amd/csrc/local_pct.hip):
  matrices, each stored as MFMA-fragment tiles [N/32][K/8][64 lanes][4]:
     lane = h*32 + j reads W[32*nt + j][h*K/2 + 4*g + e]  (the two lane halves own the two halves of K)
     0 emb1 (128 x 8, zero padded from 125 x 3)   1 emb2 (128 x 128, zero padded from 125 x 125)
     per encoder: qkv (192 x 128, LayerNorm-1 gamma folded)  out  ff1a ff1b (rows 0:128 / 128:256 of ff.linear1,
     LayerNorm-2 gamma folded)  ff2a ff2b (columns 0:128 / 128:256 of ff.linear2)
     14 lin0 (final norm gamma folded)
  vectors: emb1_b[128] emb2_b[128] | per encoder: qkv_c[192] out_b[128] ff1_c[256] ff2_b[128] | lin0_c[128]
     where c = bias + W @ beta (the LayerNorm shift folded through the linear layer).
Folding is algebraically exact; it only moves fp32 roundings (covered by the 1e-4 parity tests).
"""
import torch

from .. import _lib


def _pack(W):
    """[N, K] -> flat fragment order [N/32][K/8][64][4]."""
    N, K = W.shape
    assert N % 32 == 0 and K % 8 == 0
    t = W.reshape(N // 32, 32, 2, K // 8, 4)          # [nt, j, h, g, e]
    return t.permute(0, 3, 2, 1, 4).contiguous().reshape(-1)   # [nt, g, h, j, e]


def _pad(W, n, k):
    out = W.new_zeros(n, k)
    out[:W.shape[0], :W.shape[1]] = W
    return out


def _padv(v, n):
    out = v.new_zeros(n)
    out[:v.shape[0]] = v
    return out


def _pack_bf16x3(W):
    """[N, K] fp32 -> exact hi/mid/lo bf16 planes in the fragment order of local_pct3.hip
    [N/32][K/16][plane][64 lanes][8], returned as a float32-typed view (1.5 floats per weight).
    hi = W with the low 16 bits cleared, mid likewise from the exact remainder, lo = the exact rest: hi+mid+lo == W."""
    N, K = W.shape
    assert N % 32 == 0 and K % 16 == 0
    top = lambda t: (t.contiguous().view(torch.int32) >> 16).to(torch.int16)
    mask = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = mask(W)
    r = W - hi
    mid = mask(r)
    lo = r - mid
    assert torch.equal(hi + mid + lo, W) and torch.equal(mask(lo), lo)
    planes = torch.stack([top(hi), top(mid), top(lo)], 0)                       # [3, N, K] int16 (bf16 bit patterns)
    t = planes.reshape(3, N // 32, 32, K // 16, 2, 8)                           # [pl, nt, j, s, h, e]
    t = t.permute(1, 3, 0, 4, 2, 5).contiguous()                                # [nt, s, pl, h, j, e]
    return t.reshape(-1).view(torch.float32)


def pack_local_pct(pct, variant=1):
    """pct: macarons_amd.networks.SconeOcc.PCTransformer (default local architecture). Returns a 1-D fp32 tensor.
    variant 1: fp32 fragment image (local_pct.hip); variant 5: exact bf16 hi/mid/lo planes (local_pct5.hip);
    variant 6: fp16 hi/lo planes of the power-of-two scaled weights (local_pct6.hip); variant 7 (the opt-in 16-bit matrix path):
    the HIGH plane of variant 6's blob alone (local_pct7.hip)."""
    if variant == 5:
        return _pack_local_pct3(pct)
    if variant == 6:
        return _pack_local_pct6(pct)
    if variant == 7:
        return _pack_local_pct6(pct, planes=1)
    if variant != 1:
        raise ValueError(f"unknown fused local transformer variant {variant}")
    with torch.no_grad():
        f = lambda p: p.detach().float()
        mats, vecs = [], []
        emb = pct.embedding
        mats.append(_pack(_pad(f(emb.linear1.weight), 128, 8)))
        mats.append(_pack(_pad(f(emb.linear2.weight), 128, 128)))
        vecs += [_padv(f(emb.linear1.bias), 128), _padv(f(emb.linear2.bias), 128)]
        for enc in pct.encoders:
            g1, b1 = f(enc.norm1.weight), f(enc.norm1.bias)
            g2, b2 = f(enc.norm2.weight), f(enc.norm2.bias)
            wqkv = torch.cat((f(enc.mhsa.w_q.weight), f(enc.mhsa.w_k.weight), f(enc.mhsa.w_v.weight)), 0)
            bqkv = torch.cat((f(enc.mhsa.w_q.bias), f(enc.mhsa.w_k.bias), f(enc.mhsa.w_v.bias)), 0)
            w1, w2 = f(enc.ff.linear1.weight), f(enc.ff.linear2.weight)
            mats += [_pack(wqkv * g1[None, :]), _pack(f(enc.mhsa.out.weight)),
                     _pack((w1 * g2[None, :])[:128]), _pack((w1 * g2[None, :])[128:]),
                     _pack(w2[:, :128].contiguous()), _pack(w2[:, 128:].contiguous())]
            vecs += [bqkv + wqkv @ b1, f(enc.mhsa.out.bias), f(enc.ff.linear1.bias) + w1 @ b2, f(enc.ff.linear2.bias)]
        gn, bn = f(pct.norm.weight), f(pct.norm.bias)
        w0 = f(pct.linear0.weight)
        mats.append(_pack(w0 * gn[None, :]))
        vecs.append(f(pct.linear0.bias) + w0 @ bn)
        blob = torch.cat(mats + vecs).contiguous()
    expect = _lib.lib().mcr_local_pct_blob_floats()
    if blob.numel() != expect:
        raise RuntimeError(f"packed local transformer has {blob.numel()} floats, kernel expects {expect}")
    return blob


def _param_key(module, cache):
    """Fingerprint of a module's parameters: (identity, storage address, in-place version counter) of EVERY parameter, read from
    the live `_parameters` dicts on each call.  It therefore sees optimizer steps and load_state_dict (version), .to(device) and
    `p.data = new` (address), `layer.weight = nn.Parameter(...)` and load_state_dict(assign=True) (identity).  Only the list of
    sub-modules is collected once (walking nn.Module's recursive generators on every call cost more host time than the launches
    of an NBV step; add_module after the first forward needs invalidate()).  What no fingerprint can see is an in-place edit
    through a detached alias (`p.data.mul_()`): the pointer tables still read the live storage, but derived images (packed
    blobs, stacked QKV, split planes) need `invalidate_weight_caches()` after such an edit."""
    frozen = cache.get("frozen")
    if frozen is not None:                                   # freeze(): the owner promised not to touch the parameters
        return frozen
    mods = cache.get("mods")
    if mods is None:
        mods = cache["mods"] = [m for m in module.modules() if m._parameters]
    key = [cache.get("epoch", 0)]
    for m in mods:
        for p in m._parameters.values():
            if p is not None:
                key += (id(p), p.data_ptr(), p._version)
    return tuple(key)


def freeze(module, cache, on=True):
    """Inference mode for the fingerprint: take it ONCE now and return that key until unfreeze / invalidate -- the caller promises
    not to change the parameters meanwhile (a deployed model: weights loaded once).  Saves the ~50 us walk over the parameters in
    front of every forward's first launch."""
    cache.pop("frozen", None)
    if on:
        cache["frozen"] = _param_key(module, cache)


def invalidate(cache):
    """Forget the sub-module list (and a frozen key) and force the next key to differ (explicit invalidation hook)."""
    cache.pop("mods", None)
    cache.pop("frozen", None)
    cache["epoch"] = cache.get("epoch", 0) + 1


class BlobCache:
    """Re-pack only when a parameter changed (data_ptr / version / device).  One image per numerics variant is kept: a caller that
    alternates `ops.variant(7)` and the default per call does not re-pack on every switch."""

    def __init__(self):
        self._entries, self._c = {}, {}

    def invalidate(self):
        invalidate(self._c)

    def get(self, pct, variant=1, key=None):
        """key: a fingerprint that covers at least pct's parameters (the owner's whole-module key, taken once per forward: the three
        local transformers, the pointer table and the head planes of a SconeOcc otherwise fingerprint ~400 parameters per call,
        ~150 us of host time in front of the first launch)."""
        key = key if key is not None else _param_key(pct, self._c)
        hit = self._entries.get(variant)
        if hit is None or hit[0] != key:
            hit = self._entries[variant] = (key, pack_local_pct(pct, variant))
            for v in [v for v, e in self._entries.items() if e[0] != key]:      # images of older parameter versions: drop
                del self._entries[v]
        return hit[1]


def weight_planes(W):
    """[2, N, K] fp16 = hi | lo planes of W * 2^8 (hi = fp16(x), lo = fp16(x - hi)): what split_weights_kernel (linear3h.hip) writes per
    call, built once per parameter version for the encoders' planes GEMMs (run_encoder_planes, pct.hip)."""
    with torch.no_grad():
        x = W.detach().float() * 256.0
        hi = x.half()
        return torch.stack((hi, (x - hi.float()).half())).contiguous()


def encoder_weight_planes(enc):
    """The four plane blobs of one Encoder, in the order the C ABI reads them behind the weight table: packed QKV, out, FF 1, FF 2."""
    w, _ = enc.mhsa.packed_qkv()
    return [weight_planes(w), weight_planes(enc.mhsa.out.weight), weight_planes(enc.ff.linear1.weight), weight_planes(enc.ff.linear2.weight)]


def padded_weight_planes(W, bias, n_pad, k_pad):
    """(planes [2, n_pad, k_pad] fp16 of W * 2^8 zero-padded, bias [n_pad] fp32 zero-padded): a layer whose width is not a multiple of
    the planes GEMM's granules (the embeddings' 125 / 126-wide second layer) joins it with exact zeros (pad_weights_kernel, linear3h.hip,
    builds the same per call when the host did not)."""
    with torch.no_grad():
        n, k = W.shape
        x = torch.zeros((n_pad, k_pad), dtype=torch.float32, device=W.device)
        x[:n, :k] = W.detach().float() * 256.0
        hi = x.half()
        b = torch.zeros(n_pad, dtype=torch.float32, device=W.device)
        b[:n] = bias.detach().float()
        return torch.stack((hi, (x - hi.float()).half())).contiguous(), b.contiguous()


def planes_tail(encoders, embedding, end_weights):
    """What weight_table_with_planes() appends behind a transformer's weight_table() (include/macarons_hip.h, PLANES / END PLANES):
    four blobs per encoder, then the layers either side of the encoders -- the embedding's second layer zero-padded to 128 x 128
    (+ its padded bias) and the planes of the module's own end layers."""
    t = []
    for e in encoders:
        t += encoder_weight_planes(e)
    t += list(padded_weight_planes(embedding.linear2.weight, embedding.linear2.bias, 128, 128))
    return t + [weight_planes(W) for W in end_weights]


def table_slots(embedding, encoders, tail, offset=0):
    """{id(parameter): (table index, row slice or None)} of a transformer whose weight_table() starts at table entry `offset`: the
    embedding's four tensors, 12 entries per encoder (Encoder.weight_table: w_q / w_k / w_v are row slices of the packed qkv pair),
    then the module's own `tail` tensors."""
    slots = {id(t): (offset + k, None) for k, t in enumerate((embedding.linear1.weight, embedding.linear1.bias,
                                                              embedding.linear2.weight, embedding.linear2.bias))}
    for e, enc in enumerate(encoders):
        o = offset + 4 + 12 * e
        qk = enc.mhsa.w_q.weight.shape[0]
        rows = ((0, qk), (qk, 2 * qk), (2 * qk, 2 * qk + enc.mhsa.w_v.weight.shape[0]))
        for lin, r in zip((enc.mhsa.w_q, enc.mhsa.w_k, enc.mhsa.w_v), rows):
            slots[id(lin.weight)], slots[id(lin.bias)] = (o + 2, r), (o + 3, r)
        for k, t in enumerate((enc.norm1.weight, enc.norm1.bias)):
            slots[id(t)] = (o + k, None)
        for k, t in enumerate((enc.mhsa.out.weight, enc.mhsa.out.bias, enc.norm2.weight, enc.norm2.bias, enc.ff.linear1.weight,
                               enc.ff.linear1.bias, enc.ff.linear2.weight, enc.ff.linear2.bias)):
            slots[id(t)] = (o + 4 + k, None)
    for k, t in enumerate(tail):
        slots[id(t)] = (offset + 4 + 12 * len(encoders) + k, None)
    return slots


def grad_slots(module, slots):
    """(parameters, slots) as the HIP backwards take them: every parameter of `module` with its place in weight_table(); a parameter
    the slot map does not know is refused."""
    params = tuple(module.parameters())
    missing = [n for n, p in module.named_parameters() if id(p) not in slots]
    if missing:
        raise NotImplementedError(f"{type(module).__name__} HIP backward: parameters outside the weight table: {missing}")
    return params, tuple(slots[id(p)] for p in params)


class TableCache:
    """The weight-pointer table of a module (list of contiguous fp32 tensors + the ctypes array handed to the C ABI), rebuilt
    only when a parameter changed."""

    def __init__(self):
        self._key, self._val, self._c = None, None, {}

    def invalidate(self):
        invalidate(self._c)

    def get(self, module, build, key=None):
        key = key if key is not None else _param_key(module, self._c)
        if key != self._key:
            tensors = build()
            import ctypes
            self._val = (tensors, (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]))
            self._key = key
        return self._val


def _pack_local_pct3(pct):
    with torch.no_grad():
        f = lambda p: p.detach().float()
        mats, vecs = [], []
        emb = pct.embedding
        mats.append(_pack_bf16x3(_pad(f(emb.linear1.weight), 128, 16)))
        mats.append(_pack_bf16x3(_pad(f(emb.linear2.weight), 128, 128)))
        vecs += [_padv(f(emb.linear1.bias), 128), _padv(f(emb.linear2.bias), 128)]
        for enc in pct.encoders:
            g1, b1 = f(enc.norm1.weight), f(enc.norm1.bias)
            g2, b2 = f(enc.norm2.weight), f(enc.norm2.bias)
            wqkv = torch.cat((f(enc.mhsa.w_q.weight), f(enc.mhsa.w_k.weight), f(enc.mhsa.w_v.weight)), 0)
            bqkv = torch.cat((f(enc.mhsa.w_q.bias), f(enc.mhsa.w_k.bias), f(enc.mhsa.w_v.bias)), 0)
            w1, w2 = f(enc.ff.linear1.weight), f(enc.ff.linear2.weight)
            mats += [_pack_bf16x3(wqkv * g1[None, :]), _pack_bf16x3(f(enc.mhsa.out.weight)),
                     _pack_bf16x3((w1 * g2[None, :])[:128].contiguous()), _pack_bf16x3((w1 * g2[None, :])[128:].contiguous()),
                     _pack_bf16x3(w2[:, :128].contiguous()), _pack_bf16x3(w2[:, 128:].contiguous())]
            vecs += [bqkv + wqkv @ b1, f(enc.mhsa.out.bias), f(enc.ff.linear1.bias) + w1 @ b2, f(enc.ff.linear2.bias)]
        gn, bn = f(pct.norm.weight), f(pct.norm.bias)
        w0 = f(pct.linear0.weight)
        mats.append(_pack_bf16x3(w0 * gn[None, :]))
        vecs.append(f(pct.linear0.bias) + w0 @ bn)
        blob = torch.cat(mats + vecs).contiguous()
    expect = _lib.lib().mcr_local_pct3_blob_floats()
    if blob.numel() != expect:
        raise RuntimeError(f"packed local transformer (v3) has {blob.numel()} floats, kernel expects {expect}")
    return blob


def _pow2_scale(*Ws):
    """Power of two 2^e that brings max |W| into [2^13, 2^14): the fp16 low plane of every weight down to 2^-16 of the
    largest one is then a normal fp16 number.  Shared by matrices whose products are accumulated together."""
    m = max(float(W.abs().max()) for W in Ws)
    if m == 0.0 or not (m < float("inf")):
        return 1.0
    import math
    return 2.0 ** (13 - math.floor(math.log2(m)))


def _pack_f16x2(W, scale, planes=2):
    """[N, K] fp32 -> fp16 hi/lo planes of W * scale in the fragment order of local_pct6.hip [N/32][K/16][plane][64 lanes][8],
    returned as a float32-typed view (1 float per weight).  hi = fp16(Ws), lo = fp16(Ws - hi) (round to nearest even).
    planes=1: the high plane alone, [N/32][K/16][64 lanes][8] (local_pct7.hip; half a float per weight)."""
    N, K = W.shape
    assert N % 32 == 0 and K % 16 == 0
    Ws = W * scale                                                              # exact (power of two, no overflow: < 2^14)
    hi = Ws.to(torch.float16)
    lo = (Ws - hi.float()).to(torch.float16)
    planes = torch.stack([hi.view(torch.int16), lo.view(torch.int16)][:planes], 0)   # [planes, N, K]
    t = planes.reshape(planes.shape[0], N // 32, 32, K // 16, 2, 8)             # [pl, nt, j, s, h, e]
    t = t.permute(1, 3, 0, 4, 2, 5).contiguous()                                # [nt, s, pl, h, j, e]
    return t.reshape(-1).view(torch.float32)


# local_pct6.hip multiplies the xyz offsets by this power of two in front of their fp16 hi / lo split (lp_split.h: L6_XYZ_SCALE, the same
# value); the variant-6 blob carries the first embedding layer's bias times it and that layer's inverse scale divided by it
L6_XYZ_SCALE = 256.0


def _pack_local_pct6(pct, planes=2):
    with torch.no_grad():
        f = lambda p: p.detach().float()
        mats, vecs, inv = [], [], []

        def add(*Ws):
            sc = _pow2_scale(*Ws) if planes == 2 else 1.0     # (variant 7: weights and biases as they are, rounded to fp16)
            for W in Ws:
                mats.append(_pack_f16x2(W.contiguous(), sc, planes))
                inv.append(1.0 / sc)
            return sc
        # every bias is stored multiplied by its matrix's scale: the kernel starts the accumulator from it
        emb = pct.embedding
        s1 = add(_pad(f(emb.linear1.weight), 128, 16))
        if planes == 2:                     # the kernel's product is W 2^e (x L6_XYZ_SCALE): bias and inverse scale follow (variant 7 takes x as it is)
            s1 *= L6_XYZ_SCALE
            inv[0] /= L6_XYZ_SCALE
        s2 = add(_pad(f(emb.linear2.weight), 128, 128))
        vecs += [_padv(f(emb.linear1.bias), 128) * s1, _padv(f(emb.linear2.bias), 128) * s2]
        for enc in pct.encoders:
            g1, b1 = f(enc.norm1.weight), f(enc.norm1.bias)
            g2, b2 = f(enc.norm2.weight), f(enc.norm2.bias)
            wqkv = torch.cat((f(enc.mhsa.w_q.weight), f(enc.mhsa.w_k.weight), f(enc.mhsa.w_v.weight)), 0)
            bqkv = torch.cat((f(enc.mhsa.w_q.bias), f(enc.mhsa.w_k.bias), f(enc.mhsa.w_v.bias)), 0)
            w1, w2 = f(enc.ff.linear1.weight), f(enc.ff.linear2.weight)
            sq = add(wqkv * g1[None, :])
            so = add(f(enc.mhsa.out.weight))
            sa = add((w1 * g2[None, :])[:128])
            sb = add((w1 * g2[None, :])[128:])
            s2_ = add(w2[:, :128], w2[:, 128:])            # one exponent: both halves accumulate into the same registers
            c1 = f(enc.ff.linear1.bias) + w1 @ b2
            vecs += [(bqkv + wqkv @ b1) * sq, f(enc.mhsa.out.bias) * so, torch.cat((c1[:128] * sa, c1[128:] * sb)),
                     f(enc.ff.linear2.bias) * s2_]
        gn, bn = f(pct.norm.weight), f(pct.norm.bias)
        w0 = f(pct.linear0.weight)
        s0 = add(w0 * gn[None, :])
        vecs.append((f(pct.linear0.bias) + w0 @ bn) * s0)
        assert len(inv) == 15
        dev = mats[0].device
        fwd = [1.0 / v for v in inv]
        tail = [torch.tensor(inv + [0.0] + fwd + [0.0], dtype=torch.float32, device=dev)] if planes == 2 else []
        blob = torch.cat(mats + vecs + tail).contiguous()
    expect = _lib.lib().mcr_local_pct6_blob_floats() if planes == 2 else _lib.lib().mcr_local_pct7_blob_floats()
    if blob.numel() != expect:
        raise RuntimeError(f"packed local transformer (v{8 - planes}) has {blob.numel()} floats, kernel expects {expect}")
    return blob


def pack_head_planes(W):
    """[N, K] fp32 (K % 8 == 0) -> (planes, inv_scale): fp16 hi / lo planes of W * 2^e in the layout linear3h.hip reads,
    [plane][n][K/8][8 fp16] (returned as an int32 tensor, 4 words per 8 weights), and 2^-e.  e is chosen per matrix like the
    local-transformer blobs (_pow2_scale: max |W| lands in [2^13, 2^14)), so neither large nor small weights leave the fp16
    planes' normal range -- the kernel's own per-call split uses a fixed 2^8 and needs |w| < 255."""
    with torch.no_grad():
        W = W.detach().float().contiguous()
        N, K = W.shape
        assert K % 8 == 0
        sc = _pow2_scale(W)
        Ws = W * sc
        hi = Ws.to(torch.float16)
        lo = (Ws - hi.float()).to(torch.float16)
        planes = torch.stack((hi, lo), 0).contiguous().view(torch.int32)        # [2, N, K/2] int32 = [2][N][K/8][4 words]
    return planes, 1.0 / sc


class HeadPlaneCache:
    """The pre-split planes of SconeOcc's four large head matrices (x_embedding.linear2 / linear3, linear1[:, 512:], linear2),
    rebuilt when a parameter changes.  get() -> (tensors kept alive, ctypes void* array[4], ctypes float array[4])."""

    def __init__(self):
        self._key, self._val, self._c = None, None, {}

    def invalidate(self):
        invalidate(self._c)

    def get(self, occ, key=None):
        key = key if key is not None else _param_key(occ, self._c)
        if key != self._key:
            import ctypes
            g = occ.global_feature_dim
            mats = [occ.x_embedding.linear2.weight, occ.x_embedding.linear3.weight, occ.linear1.weight[:, g:], occ.linear2.weight]
            packed = [pack_head_planes(W) for W in mats]
            self._val = ([p for p, _ in packed], (ctypes.c_void_p * 4)(*[p.data_ptr() for p, _ in packed]),
                         (ctypes.c_float * 4)(*[inv for _, inv in packed]))
            self._key = key
        return self._val
