"""Host-side mirror of macarons/networks/SconeOcc.py: the occupancy-probability network, running on the
MI355X through libmacarons_hip.so.  Same constructors, parameter names and tensor layouts as the reference
(XEmbedding :7, PCTransformer :45, SconeOcc :133, forward :250).

Hidden RNG: SconeOcc.forward draws torch.randperm on the CPU default generator three times
(SconeOcc.py:269 and :311 twice).  This class draws them on the host in the same order, or takes them
explicitly through `perms=` so tests can pin them.
"""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F          # noqa: F401  (not used here: a public name of upstream's module, tests/test_patch_reference.py)
from torch import nn

from .. import autograd as A
from .. import ops, _lib
from .Attention import (Embedding, Encoder, FeedForward, MultiHeadSelfAttention, attention, knn_gather,   # noqa: F401
                        _f32c, _inference_only)     # the public ones are what upstream's `from .Attention import *` hands on
from ..utility.utils import get_knn_points   # noqa: F401  (SconeOcc.py:4)
from ..utility.host import batched_draws_ok, native_op
from .packing import (BlobCache, HeadPlaneCache, TableCache, _param_key, grad_slots, planes_tail, table_slots, invalidate as _invalidate_key,
                      freeze as _freeze_key)
from .range_guard import RangeGuard


class XEmbedding(nn.Module):
    """SconeOcc.py:7-42: 3 -> E/4 -> E/2 -> E with GELU after every layer."""

    def __init__(self, x_dim, x_embedding_dim, dropout=None, gelu=True):
        super().__init__()
        if not gelu or dropout is not None:
            raise NotImplementedError("HIP path implements the GELU / no-dropout configuration")
        self.linear1 = nn.Linear(x_dim, x_embedding_dim // 4)
        self.linear2 = nn.Linear(x_embedding_dim // 4, x_embedding_dim // 2)
        self.linear3 = nn.Linear(x_embedding_dim // 2, x_embedding_dim)
        self.non_linear1, self.non_linear2, self.non_linear3 = nn.GELU(), nn.GELU(), nn.GELU()
        self.dropout = None

    def forward(self, x):
        _inference_only(self, x)
        res = ops.linear(x, _f32c(self.linear1.weight), _f32c(self.linear1.bias), gelu=True)
        res = ops.linear(res, _f32c(self.linear2.weight), _f32c(self.linear2.bias), gelu=True)
        return ops.linear(res, _f32c(self.linear3.weight), _f32c(self.linear3.bias), gelu=True)


def _native_ragged_tables():
    """Is torch.ops.macarons.ragged_tables there (the C++ extension built)?  MCR_NATIVE_RAGGED_TABLES=0: ragged_job_tables (A/B, tests)."""
    return native_op("ragged_tables", "MCR_NATIVE_RAGGED_TABLES")      # (read from os.environ there, once)


def ragged_job_tables(cloud_sizes, query_sizes, rows, with_row_job):
    """The tables a ragged pass uploads in front of its first launch, as one int64 array (what torch.ops.macarons.ragged_tables builds in
    one C++ loop): cloud offsets [J + 1] | one (job, first query row, rows, 0) record per block of `rows` queries | with_row_job: the
    job of every query row [T].  A job without queries has no block."""
    J = len(cloud_sizes)
    off0 = np.concatenate(([0], np.cumsum(cloud_sizes))).astype(np.int64)
    qs = np.asarray(query_sizes, np.int64)
    q0 = np.concatenate(([0], np.cumsum(qs)))
    nb = -(-qs // rows)                                              # query blocks per job
    bj = np.repeat(np.arange(J, dtype=np.int64), nb)                 # job of every block
    b_in = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)     # block index inside its job
    blocks = np.stack((bj, q0[bj] + b_in * rows, np.minimum(rows, qs[bj] - b_in * rows), np.zeros_like(bj)), 1)
    parts = [off0, blocks.reshape(-1)]
    if with_row_job:
        parts.append(np.repeat(np.arange(J, dtype=np.int64), qs))
    return np.concatenate(parts)


def ragged_index_arrays(perms, off0, J, Lg):
    """The index arrays of a ragged pass's down-sampled clouds from given draws (per job the three index tensors of draw_perms), as
    one int64 array (what torch.ops.macarons.scone_occ_draws returns for its own draws): g_idx [J, Lg] | idx1 | idx2 | off1 [J + 1] |
    off2 [J + 1] | global_len [J].  off0: the clouds' offsets [J + 1]."""
    p0s = [np.asarray(p[0], dtype=np.int64)[:Lg] for p in perms]
    p1s = [np.asarray(p[1], dtype=np.int64) for p in perms]
    p2s = [np.asarray(p[2], dtype=np.int64) for p in perms]
    n0 = np.asarray([len(p) for p in p0s], np.int64)
    n1 = np.asarray([len(p) for p in p1s], np.int64)
    n2 = np.asarray([len(p) for p in p2s], np.int64)
    off1 = np.concatenate(([0], np.cumsum(n1)))
    off2 = np.concatenate(([0], np.cumsum(n2)))
    g_idx = np.repeat(off0[:J], Lg).reshape(J, Lg)                # padding rows: any valid point (masked by global_len)
    col = np.arange(int(n0.sum()), dtype=np.int64) - np.repeat(np.cumsum(n0) - n0, n0)
    g_idx[np.repeat(np.arange(J), n0), col] = np.concatenate(p0s) + np.repeat(off0[:J], n0)
    idx1 = np.concatenate(p1s) + np.repeat(off0[:J], n1)
    idx2 = np.concatenate(p2s) + np.repeat(off1[:J], n2)          # scale 2 indexes scale 1's rows (SconeOcc.py:311)
    return np.concatenate([g_idx.reshape(-1), idx1, idx2, off1, off2, n0])


@dataclasses.dataclass(slots=True)
class _Begun:
    """Handle of forward_begin (opaque to callers): the contiguous inputs phase 1 ran on, and what forward(begun=) checks before it
    trusts them."""
    pc: torch.Tensor
    x: torch.Tensor
    variant: int
    sizes: list
    src: tuple
    epoch: int


@dataclasses.dataclass(slots=True)
class _RaggedPass:
    """Handle of forward_ragged_begin (opaque to callers): the inputs, the uploaded tables, the pass's memo of weight images per
    variant (`images`), and the epoch of the arena that holds phase 1's results (`epoch1`, known once phase 1 is queued)."""
    pc: torch.Tensor
    x: torch.Tensor
    vh: torch.Tensor
    variant: int
    cloud_sizes: list
    query_sizes: list
    off0: np.ndarray
    d_off0: torch.Tensor
    d_row_job: torch.Tensor
    d_blocks: torch.Tensor
    arena: str
    images: dict = dataclasses.field(default_factory=dict)
    epoch1: int = None


class PCTransformer(nn.Module):
    """SconeOcc.py:45-130."""

    def __init__(self, seq_len, pts_dim=3, pts_embedding_dim=256, feature_dim=512, concatenate_input=True, n_code=2,
                 n_heads=4, FF=True, gelu=True, dropout=None):
        super().__init__()
        self.seq_len, self.pts_dim, self.pts_embedding_dim = seq_len, pts_dim, pts_embedding_dim
        self.n_code, self.n_heads, self.FF, self.gelu = n_code, n_heads, FF, gelu
        self.feature_dim = feature_dim
        self.dropout = dropout
        self.embedding = Embedding(input_dim=pts_dim, output_dim=pts_embedding_dim, dropout=None, gelu=gelu,
                                   global_feature=False, additional_feature_dim=0, concatenate_input=concatenate_input,
                                   k_for_knn=0)
        self.encoders = nn.ModuleList([Encoder(seq_len=seq_len, embedding_dim=pts_embedding_dim,
                                               qk_dim=pts_embedding_dim // 4, n_heads=n_heads, dropout=dropout, gelu=gelu,
                                               FF=FF) for _ in range(n_code)])
        self.norm = nn.LayerNorm(pts_embedding_dim)
        self.linear0 = nn.Linear(pts_embedding_dim, feature_dim // 2)

    def _is_default_arch(self):
        return (self.pts_dim == 3 and self.pts_embedding_dim == 128 and self.n_code == 2 and self.n_heads == 4
                and self.FF and self.embedding.concatenate_input and self.feature_dim in (256, 512))

    def weight_table(self):
        t = [_f32c(self.embedding.linear1.weight), _f32c(self.embedding.linear1.bias),
             _f32c(self.embedding.linear2.weight), _f32c(self.embedding.linear2.bias)]
        for e in self.encoders:
            t += e.weight_table()
        t += [_f32c(self.norm.weight), _f32c(self.norm.bias), _f32c(self.linear0.weight), _f32c(self.linear0.bias)]
        return t

    def _grad_slots(self):
        """(parameters, slots): every parameter of the module with its place in weight_table() -- (table index, row slice or None);
        w_q / w_k / w_v are rows 0:32 / 32:64 / 64:192 of their encoder's packed qkv entries."""
        return grad_slots(self, table_slots(self.embedding, self.encoders, (self.norm.weight, self.norm.bias, self.linear0.weight,
                                                                            self.linear0.bias)))

    def forward(self, pc, mask=None):
        """pc [n_clouds, seq_len, 3] -> [n_clouds, feature_dim].  Differentiable (once) without a mask: HIP forward, HIP backward
        (autograd.PCTransformerFunction); the mask= path is inference only."""
        if mask is None and self._is_default_arch() and A.needs_grad(self, pc):
            params, slots = self._grad_slots()
            return A.PCTransformerFunction.apply(self._forward_hip, self.weight_table, slots, self.feature_dim, pc, *params)
        return self._forward_hip(pc, mask)

    def _forward_hip(self, pc, mask=None):
        _inference_only(self, pc)
        if not self._is_default_arch():
            raise NotImplementedError("the fused MI355X PCTransformer implements the reference's default architecture")
        if mask is not None:                            # SconeOcc.py:106-118: the mask goes to every encoder; block by block (see SconeVis.forward)
            x = self.embedding(pc)
            for enc in self.encoders:
                x = enc(x, mask=mask)
            x = ops.linear(ops.layernorm(x, _f32c(self.norm.weight), _f32c(self.norm.bias)), _f32c(self.linear0.weight), _f32c(self.linear0.bias))
            return ops.pool_max_avg(x)
        if pc.shape[1] >= 512:                          # long sequences: planes of every GEMM's weights, built once per parameter version
            if not hasattr(self, "_table_cache"):
                self._table_cache = TableCache()
            return ops.pc_transformer_forward(pc, self._table_cache.get(self, self.weight_table_with_planes), self.feature_dim)
        return ops.pc_transformer_forward(pc, self.weight_table(), self.feature_dim)

    def weight_table_with_planes(self):
        """weight_table() + the encoders' weights as fp16 hi/lo planes (8 blobs) + the end layers' (3): packing.planes_tail."""
        return self.weight_table() + planes_tail(self.encoders, self.embedding, (self.linear0.weight,))


class SconeOcc(RangeGuard, nn.Module):
    def __init__(self, seq_len=2048, pts_dim=3, pts_embedding_dim=128, concatenate_input=True, n_code=2, n_heads=4,
                 FF=True, gelu=True, global_feature_dim=512, n_scale=3, local_feature_dim=256, k_for_knn=16, x_dim=3,
                 x_embedding_dim=512, n_harmonics=64, output_dim=1, dropout=None, offset=True):
        super().__init__()
        self.seq_len, self.pts_dim, self.pts_embedding_dim = seq_len, pts_dim, pts_embedding_dim
        self.n_code, self.n_heads, self.FF, self.gelu = n_code, n_heads, FF, gelu
        self.n_scale = n_scale
        self.x_dim, self.x_embedding_dim = x_dim, x_embedding_dim
        self.output_dim = output_dim
        self.dropout = dropout
        self.encoding_dim = pts_embedding_dim
        self.k_for_knn = k_for_knn
        self.offset = offset
        if self.offset:
            print("Offset set to True.")                                     # SconeOcc.py:199-200
        self.global_feature_dim, self.local_feature_dim = global_feature_dim, local_feature_dim
        self.n_harmonics = n_harmonics
        self.all_feature_size = x_embedding_dim + n_scale * local_feature_dim + global_feature_dim + n_harmonics
        self.global_transformer = PCTransformer(seq_len=seq_len, pts_dim=pts_dim, pts_embedding_dim=pts_embedding_dim,
                                                feature_dim=global_feature_dim, concatenate_input=concatenate_input,
                                                n_code=n_code, n_heads=n_heads, FF=FF, gelu=gelu, dropout=dropout)
        self.local_transformers = nn.ModuleList([
            PCTransformer(seq_len=k_for_knn, pts_dim=pts_dim, pts_embedding_dim=pts_embedding_dim,
                          feature_dim=local_feature_dim, concatenate_input=concatenate_input, n_code=n_code,
                          n_heads=n_heads, FF=FF, gelu=gelu, dropout=dropout) for _ in range(n_scale)])
        self.x_embedding = XEmbedding(x_dim=x_dim, x_embedding_dim=x_embedding_dim, dropout=dropout, gelu=gelu)
        self.linear1 = nn.Linear(self.all_feature_size, 512)
        self.linear2 = nn.Linear(512, 256)
        self.linear3 = nn.Linear(256, output_dim)
        self.non_linear1, self.non_linear2, self.non_linear3 = nn.GELU(), nn.GELU(), nn.GELU()
        # fused LDS-resident local transformers (local_pct.hip); set False to run them layer by layer
        self.fused_local = True
        self._blob_caches = [BlobCache() for _ in range(n_scale)]
        self._table_cache = TableCache()
        self._head_cache = HeadPlaneCache()
        self._key_cache = {}

    def freeze_weight_caches(self, on=True):
        """Inference mode: fingerprint the parameters once, now, and trust them unchanged until freeze_weight_caches(False) or
        invalidate_weight_caches() (an optimizer step or load_state_dict in between would go unnoticed: opt-in)."""
        _freeze_key(self, self._key_cache, on)

    def invalidate_weight_caches(self):
        """Drop every derived weight image (pointer table, packed local-transformer blobs, stacked QKV, split head planes): call
        after editing parameters in a way no fingerprint can see (in place through `p.data`, see packing._param_key)."""
        _invalidate_key(self._key_cache)                             # the shared per-forward fingerprint: every cache below rebuilds
        self._table_cache.invalidate()
        self._head_cache.invalidate()
        for c in self._blob_caches:
            c.invalidate()
        for m in self.modules():
            if hasattr(m, "_packed"):
                m._packed = None

    def _is_default_arch(self):
        return (self.n_scale == 3 and self.k_for_knn == 16 and self.offset and self.x_dim == 3 and self.x_embedding_dim == 512
                and self.global_feature_dim == 512 and self.local_feature_dim == 256 and self.n_harmonics == 64
                and self.output_dim == 1 and self.global_transformer._is_default_arch()
                and all(t._is_default_arch() for t in self.local_transformers))

    def weight_table(self):
        t = self.global_transformer.weight_table()
        for lt in self.local_transformers:
            t += lt.weight_table()
        for lin in (self.x_embedding.linear1, self.x_embedding.linear2, self.x_embedding.linear3, self.linear1,
                    self.linear2, self.linear3):
            t += [_f32c(lin.weight), _f32c(lin.bias)]
        return t

    def _grad_slots(self):
        """(parameters, slots): every parameter of the module with its place in weight_table() -- (table index, row slice or None); the
        four transformers' w_q / w_k / w_v are rows 0:32 / 32:64 / 64:192 of their encoder's packed qkv entries."""
        slots, o = {}, 0
        for t in (self.global_transformer, *self.local_transformers):
            ps, sl = t._grad_slots()
            for p_, (k, rows) in zip(ps, sl):
                slots[id(p_)] = (o + k, rows)
            o += len(t.weight_table())
        for lin in (self.x_embedding.linear1, self.x_embedding.linear2, self.x_embedding.linear3, self.linear1, self.linear2,
                    self.linear3):
            slots[id(lin.weight)], slots[id(lin.bias)] = (o, None), (o + 1, None)
            o += 2
        return grad_slots(self, slots)

    def weight_table_with_planes(self):
        """weight_table() + the global transformer's encoder weights as fp16 hi/lo planes (8 blobs) and its end layers' (3)."""
        g = self.global_transformer
        return self.weight_table() + planes_tail(g.encoders, g.embedding, (g.linear0.weight,))

    def ds_factor(self, full_seq_len):
        """SconeOcc.py:281-288."""
        if self.n_scale > 1:
            ds = int(np.power(full_seq_len / (self.k_for_knn * 8), 1. / (self.n_scale - 1)))
            return 2 if ds == 0 else ds
        return 1

    def draw_perms(self, full_seq_len):
        """The three torch.randperm draws of one forward, in the reference's order on the CPU default generator:
        global down-sample (SconeOcc.py:269), then scale 0->1 and 1->2 (:311).  Returns index tensors (already cut)."""
        perms = [torch.randperm(full_seq_len)[:self.seq_len]]
        ds, m = self.ds_factor(full_seq_len), full_seq_len
        for _ in range(self.n_scale - 1):
            perms.append(torch.randperm(m)[:m // ds])
            m = m // ds
        return perms

    @staticmethod
    def _take(pc, p):
        """pc[:, p] for a shared 1-D index (SconeOcc.py:269, :311) or, extension, a per-cloud [n_clouds, n] index (a scene batch in
        which every object keeps the draws its own single-cloud call would have made)."""
        p = p.to(pc.device)
        if p.dim() == 1:
            return pc[:, p].contiguous()
        return torch.gather(pc, 1, p[..., None].expand(-1, -1, pc.shape[-1])).contiguous()

    def forward_ragged(self, pc, cloud_sizes, x, view_harmonics, query_sizes, perms=None, index_arrays=None, out=None,
                       differentiable=False):
        """J forward() calls of different sizes as ONE launch sequence (extension; the reference calls forward once per grid cell and
        chunk from a Python loop, macarons_utils.py:1395-1540).  Job j: surface cloud = the next cloud_sizes[j] rows of pc [sum M, 3],
        queries = the next query_sizes[j] rows of x [T,3] / view_harmonics [T,64] (host lists).  perms: per job the three index
        tensors draw_perms(cloud_sizes[j]) returns; None = drawn here in job order on the CPU generator, exactly the draws J
        sequential forward() calls would make; index_arrays: the uploaded index arrays of an earlier pass (`last_ragged_perms`: a
        caller that repeats a pass, or hands rank 0's draws to every rank).
        -> [T,1] (`out`: written there).  = forward_ragged_begin + forward_ragged_finish.
        differentiable=True, with gradients enabled and a parameter, x or view_harmonics requiring one: the result carries ONE autograd
        node (autograd.SconeOccRaggedFunction) whose backward is HIP end to end -- the three scales' offsets, then
        mcr_scone_occ_backward_ragged over the rows of all jobs, weight gradients summed over the jobs; the values are the bits of the
        call without the keyword on the same draws (the same launches, without the range flag, as forward() under
        MCR_SCONE_OCC_BWD=hip; that variable is not consulted here).  The clouds get no gradient: pc.requires_grad is refused
        (NotImplementedError), and so is out= (ValueError).  Without the keyword, under no_grad or with nothing requiring a gradient
        the call builds no graph."""
        self._check_differentiable(differentiable, pc, out)
        h = self.forward_ragged_begin(pc, cloud_sizes, x, view_harmonics, query_sizes)
        return self.forward_ragged_finish(h, perms=perms, index_arrays=index_arrays, out=out, differentiable=differentiable)

    @staticmethod
    def _check_differentiable(differentiable, pc, out):
        if not differentiable:
            return
        if pc.requires_grad:
            raise NotImplementedError("forward_ragged(differentiable=True): the clouds get no gradient on this path (pc.requires_grad)")
        if out is not None:
            raise ValueError("forward_ragged(differentiable=True) returns a new tensor that carries the graph: out= cannot be given")

    def forward_ragged_begin(self, pc, cloud_sizes, x, view_harmonics, query_sizes, row_job=None, arena="scone_occ_ragged"):
        """First half of forward_ragged: what needs no hidden draw is uploaded and LAUNCHED (phase 1: the x embedding, the scale-0 search
        and local transformer on the whole clouds), so that the GPU works while the host makes the ~3 J torch.randperm draws
        (forward_ragged_finish).  row_job (int32 device [T], optional): the job of every query row when the caller already holds it.
        arena: tag of the scratch arena that keeps phase 1's results until the finish (several begun passes need one each)."""
        if not self._is_default_arch() or not self.fused_local:
            raise NotImplementedError("forward_ragged implements the default architecture on the fused local-transformer path")
        dev = x.device
        J = len(cloud_sizes)
        pc = pc.contiguous()
        rows = int(_lib.lib().mcr_knn_rows_per_block())
        if _native_ragged_tables():                                      # one C++ loop (this runs in front of the pass's first launch)
            host = torch.ops.macarons.ragged_tables([int(m) for m in cloud_sizes], [int(q) for q in query_sizes], rows, row_job is None)
        else:
            host = torch.from_numpy(ragged_job_tables(cloud_sizes, query_sizes, rows, row_job is None))
        n_blk4 = host.numel() - (J + 1) - (sum(int(q) for q in query_sizes) if row_job is None else 0)
        early = ops.h2d(host, torch.int64, dev)
        h = _RaggedPass(pc=pc, x=x, vh=view_harmonics, variant=ops.current_variant(), cloud_sizes=cloud_sizes,
                        query_sizes=query_sizes, off0=host[:J + 1].numpy(), d_off0=early[:J + 1],
                        d_blocks=early[J + 1:J + 1 + n_blk4].to(torch.int32).view(-1, 4),
                        d_row_job=early[J + 1 + n_blk4:].to(torch.int32) if row_job is None else row_job, arena=arena)
        with torch.no_grad():
            self._ragged_phase1(h, h.variant)
        h.epoch1 = ops.scone_occ_epoch(dev, arena)
        return h

    def _ragged_phase1(self, h, v):
        table, blobs, head = self._images(v, h.images)
        ops.scone_occ_forward_ragged(None, None, [h.pc], [h.d_off0], h.x, h.vh, h.d_row_job, h.d_blocks, table, blobs, head, None,
                                     phase=1, Lg=self.seq_len, arena=h.arena)

    def _ragged_index_arrays(self, h, perms):
        """The uploaded index arrays of the pass's down-sampled clouds (`last_ragged_perms`) from `perms`, or from draws made here."""
        J, Lg = len(h.cloud_sizes), self.seq_len
        if perms is None and not batched_draws_ok():                     # torch.randperm was replaced from Python: honour it
            perms = [self.draw_perms(int(m)) for m in h.cloud_sizes]
        if perms is None:
            # the 3 J draws in job order on the CPU generator -- exactly the draws J sequential forward() calls make -- by ONE call
            # into the C++ extension (the same at::randperm calls; no dispatcher round trip and no numpy per draw), which returns
            # the index arrays ready to upload
            from .. import torch_ops  # noqa: F401
            sz = [self.scale_sizes(int(m)) for m in h.cloud_sizes]
            flat = torch.ops.macarons.scone_occ_draws([s_[0] for s_ in sz], [s_[1] for s_ in sz], [s_[2] for s_ in sz], Lg)
            n1, n2 = sum(s_[1] for s_ in sz), sum(s_[2] for s_ in sz)
        else:
            flat = ragged_index_arrays(perms, h.off0, J, Lg)
            n1, n2 = sum(len(p[1]) for p in perms), sum(len(p[2]) for p in perms)
        d = ops.h2d(flat, torch.int64, h.x.device)                       # ONE upload
        cut, o = [], 0
        for n in (J * Lg, n1, n2, J + 1, J + 1, J):
            cut.append(d[o:o + n]); o += n
        return {"g_idx": cut[0], "idx1": cut[1], "idx2": cut[2], "off1": cut[3], "off2": cut[4], "g_len": cut[5].to(torch.int32)}

    def forward_ragged_finish(self, h, perms=None, index_arrays=None, out=None, differentiable=False):
        """Second half of forward_ragged: the hidden draws (unless given), the down-sampled clouds, phase 2.  differentiable: see
        forward_ragged."""
        self._check_differentiable(differentiable, h.pc, out)
        pc, x, view_harmonics, variant, dev = h.pc, h.x, h.vh, h.variant, h.x.device
        ia = index_arrays if index_arrays is not None else self._ragged_index_arrays(h, perms)
        self.last_ragged_perms = ia         # (a caller that repeats the pass -- on another variant, on another rank -- re-uses the draws: index_arrays=)
        pc_global = pc[ia["g_idx"]].view(len(h.cloud_sizes), self.seq_len, 3)
        pc1 = pc[ia["idx1"]]
        pc2 = pc1[ia["idx2"]]

        def run(v, flag, redo_phase1, out_):
            if redo_phase1:
                self._ragged_phase1(h, v)
            table, blobs, head = self._images(v, h.images)
            return ops.scone_occ_forward_ragged(pc_global, ia["g_len"], [pc, pc1, pc2], [h.d_off0, ia["off1"], ia["off2"]], x, view_harmonics,
                                                h.d_row_job, h.d_blocks, table, blobs, head, flag, phase=2, out=out_, arena=h.arena)

        # (phase 1's results live in the stream's arena: if anything else wrote it since -- another thread on this stream -- redo it)
        stale = lambda: ops.scone_occ_epoch(dev, h.arena) != h.epoch1       # noqa: E731
        if differentiable and A.needs_grad(self, x, view_harmonics):
            # HIP forward (the launches above, no range flag), HIP backward: one node over the rows of all jobs
            params, slots = self._grad_slots()
            sz = [self.scale_sizes(int(m)) for m in h.cloud_sizes]
            return A.SconeOccRaggedFunction.apply(
                lambda: run(variant, None, stale(), None), self.weight_table, slots,
                [[s_[i] for s_ in sz] for i in range(self.n_scale)], h.query_sizes, pc_global, ia["g_len"], [pc, pc1, pc2], h.d_row_job,
                x, view_harmonics, *params)
        guard = self._effective_guard()
        flag = self._arm_range(dev, guard) if variant in (6, 7) and guard != "off" else None
        with torch.no_grad():
            res = run(variant, flag, stale(), out)
            redo = self._settle_range(flag, guard, lambda: run(5, None, True, out))
        return res if redo is None else redo

    def scale_sizes(self, full_seq_len):
        """Points of the three neighbourhood clouds of a forward on a cloud of full_seq_len points (SconeOcc.py:282-288, :311)."""
        ds, sizes = self.ds_factor(full_seq_len), [full_seq_len]
        for _ in range(self.n_scale - 1):
            sizes.append(sizes[-1] // ds)
        return sizes

    def _images(self, variant, memo=None):
        """(table, blobs, head): the weight images of a variant -- pointer table with planes, packed local-transformer blobs, split head
        planes -- each rebuilt only when the parameters' fingerprint changed.  memo (a ragged pass's dict): one fingerprint walk per
        variant per PASS rather than per call (host time in front of the pass's launches)."""
        if memo is not None and variant in memo:
            return memo[variant]
        key = _param_key(self, self._key_cache)                     # one fingerprint of the parameters for every derived image
        blobs = [c.get(t, variant, key) for c, t in zip(self._blob_caches, self.local_transformers)] if self.fused_local else None
        head = self._head_cache.get(self, key) if variant in (6, 7) else None
        images = (self._table_cache.get(self, self.weight_table_with_planes, key), blobs, head)
        if memo is not None:
            memo[variant] = images
        return images

    def forward_begin(self, pc, x):
        """Extension: queue the part of forward(pc, x, ...) that needs neither the view harmonics nor the hidden draws (the query
        order of the neighbour search, scale 0: search + local transformer over the whole cloud) and return a handle for
        forward(..., begun=handle), which then runs the rest.  A caller that still has host work to do before it can call forward --
        view state, harmonics, down-sampled clouds (nbv_step) -- hides that work behind this first long kernel.  None (and nothing
        queued) when the split does not apply (gradients wanted, non-default architecture, layer-by-layer path)."""
        if not self._is_default_arch() or not self.fused_local or A.needs_grad(self, pc, x):
            return None
        variant = ops.current_variant()
        pc0, x_ = pc.contiguous(), x.contiguous()
        sizes = self.scale_sizes(pc.shape[1])
        if min(sizes) < self.k_for_knn:
            return None
        with torch.no_grad():
            table, blobs, head = self._images(variant)
            ops.scone_occ_forward(None, [pc0, None, None], x_, None, table, blobs, head, None, phase=1, M_scale=sizes, Lg=self.seq_len)
        return _Begun(pc=pc0, x=x_, variant=variant, sizes=sizes, src=(pc, x), epoch=ops.scone_occ_epoch(pc0.device, "scone_occ"))

    def forward(self, pc, x, view_harmonics, mask=None, verbose=False, perms=None, begun=None):
        """pc [n_clouds, M, 3], x [n_clouds, Q, 3], view_harmonics [n_clouds, Q, 64] -> [n_clouds, Q, 1].
        `perms` (optional): the three index tensors draw_perms() would return, to pin the hidden RNG; each either 1-D (shared by
        the clouds, as the reference draws them) or [n_clouds, n] (one draw per cloud).  `begun`: the handle of forward_begin(pc, x)
        (same tensors): only the remaining part runs."""
        if mask is not None:
            # upstream hands ONE mask to the 2048-token global transformer and to the 16-token local ones (SconeOcc.py:271, :301): no
            # shape fits both, so no caller can pass one; PCTransformer.forward(mask=...) itself is supported
            raise NotImplementedError("SconeOcc.forward(mask=...): upstream applies the same mask to sequences of 2048 and of 16 tokens")
        if not self._is_default_arch():
            raise NotImplementedError("the fused MI355X SconeOcc forward implements the reference's default architecture")
        n_clouds, full_seq_len = pc.shape[0], pc.shape[1]
        n_sample = x.shape[1]
        if perms is None:
            perms = self.draw_perms(full_seq_len)
        dev = pc.device
        if self._range_reenter():
            with ops.variant(5):
                return self.forward(pc, x, view_harmonics, mask, verbose, perms, None)
        variant = ops.current_variant()
        # A handle of forward_begin is valid only for the very tensors, numerics and cloud sizes it was queued with -- and only while
        # nothing else has written the arena that holds its phase-1 results (ops.scone_occ_epoch).  Checked BEFORE anything of the
        # handle is used: a stale or foreign handle is ignored and the whole forward runs on `pc` / `x`.
        sizes = self.scale_sizes(full_seq_len)
        if begun is not None and not (begun.src[0] is pc and begun.src[1] is x and begun.variant == variant
                                      and begun.sizes == sizes and [p_.shape[-1] for p_ in perms] == [self.seq_len] + sizes[1:]
                                      and begun.epoch == ops.scone_occ_epoch(dev, "scone_occ")):
            begun = None
        pc_global = self._take(pc, perms[0])                                          # SconeOcc.py:269
        scales = [begun.pc if begun is not None else pc.contiguous()]
        for p in perms[1:]:
            scales.append(self._take(scales[-1], p))                                  # :311
        phase = 0
        if begun is not None:
            phase, x = 2, begun.x

        def run(variant, pc_global, scales, x_, vh_, flag, phase=0):
            table, blobs, head = self._images(variant)
            return ops.scone_occ_forward(pc_global, scales, x_, vh_, table, blobs, head, flag, phase=phase)

        guard = self._effective_guard()
        flag = self._arm_range(dev, guard) if variant in (6, 7) and guard != "off" else None
        if A.needs_grad(self, pc, x, view_harmonics) and A.scone_occ_backward_mode() == "hip" and not pc.requires_grad:
            # HIP forward, HIP backward (autograd.SconeOccFunction); a gradient for the surface points takes the `pct` route below
            params, slots = self._grad_slots()
            res = A.SconeOccFunction.apply(lambda g_, sc_, x_, vh_: run(variant, g_, sc_, x_, vh_, None), self.weight_table, slots,
                                           self.k_for_knn, pc_global, scales, x, view_harmonics, *params)
        elif A.needs_grad(self, pc, x, view_harmonics):   # trainers: HIP forward, composite-torch backward (autograd.py)
            pidx = [p.to(dev) for p in perms]

            def clouds(pc_):
                sc = [pc_.contiguous()]
                for p in pidx[1:]:
                    sc.append(self._take(sc[-1], p))
                return self._take(pc_, pidx[0]), sc

            def hip(pc_, x_, vh_):
                g, sc = clouds(pc_)
                return run(variant, g, sc, x_, vh_, None)

            def composite(pc_, x_, vh_):
                g, sc = clouds(pc_)
                with torch.no_grad():
                    idx = [ops.knn_points(x_.detach().contiguous(), s_.detach(), self.k_for_knn)[2] for s_ in sc]
                return A.scone_occ(self, g, sc, x_, vh_, idx)
            res = A.with_torch_backward(hip, composite, (pc, x, view_harmonics), self)
        else:
            res = run(variant, pc_global, scales, x, view_harmonics, flag, phase)
            redo = self._settle_range(flag, guard, lambda: run(5, pc_global, scales, x, view_harmonics, None))
            res = res if redo is None else redo                         # (out of the fp16 range: the full-range result)
        return res.view(n_clouds, n_sample, self.output_dim)
