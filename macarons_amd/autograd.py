"""Gradients for the trainers (`loss.backward()` through SconeVis.forward / compute_coverage_gain at
macarons/trainers/pretrain_scone_vis.py:224, through SconeOcc.forward at pretrain_scone_occ.py, train_macarons.py:1159-1162).

The forward passes stay on the hand-written HIP kernels.  SconeVis.forward's backward is HIP too (SconeVisFunction below:
mcr_scone_vis_backward, scone_vis_bwd.hip), as is the scorer's (the Autograd kernels of torch.ops.macarons.sh_coverage_gain /
sh_visibilities) and that of PCTransformer.forward called on its own (PCTransformerFunction below: mcr_pc_transformer_backward, pct_bwd.hip).
SconeOcc's entry point is still wrapped in a torch.autograd.Function whose backward RECOMPUTES the same
mathematics with plain torch ops on the same device (composite functions below, written against the modules' own parameters) under
autograd and back-propagates through that; env MCR_SCONE_VIS_BWD=composite puts SconeVis back on that path (A/B).  Opt-in, env
MCR_SCONE_OCC_BWD=pct: that recomputation evaluates SconeOcc's four PCTransformers -- almost all of its work -- through
PCTransformerFunction (HIP forward and backward); the gather, the offsets, the x-embedding and the head stay torch.  Opt-in,
MCR_SCONE_OCC_BWD=hip: no recomputation in torch at all -- SconeOccFunction below hands the whole backward (gather, local transformers,
x-embedding, head, global transformer) to one entry, mcr_scone_occ_backward, for the parameters, x and the view harmonics; a gradient
for the surface points pc is not computed there, so a forward whose pc requires one takes the pct route.  The MACARONS-regime gain
(ops.macarons_gain_indexed / macarons_gain_) is HIP both ways as well: MacaronsGainFunction below, backward mcr_macarons_gain_backward, with
gradients for the per-point visibility gains and the volumes and for nothing else.  The depth module's plane sweep (ops.cost_volume)
is HIP both ways too (CostVolumeFunction below: mcr_cost_volume_backward; env MCR_COST_VOLUME_BWD=composite puts it back on the
recomputation through networks.ManyDepth.cost_volume_planes, A/B), and so is the depth module's photometric reconstruction loss
(ReconstructionLossFunction: mcr_reconstruction_loss_backward, for the depth alone; env MCR_RECONSTRUCTION_LOSS_BWD=composite) and the step
in front of it, from the network's disparity maps to the depths, regularity values and error mask (DisparityScalesFunction:
mcr_disparity_scales_backward, for the disparities alone; env MCR_DISPARITY_SCALES_BWD=composite).  The composites
are ordinary differentiable torch code, so they are also what the parity tests differentiate numerically (tests/test_autograd.py:
fp64 finite differences on CPU; on the GPU the composite forward must reproduce the HIP forward to 1e-4, which makes its gradient
the gradient of the kernels' function) and the second reference of the HIP backward's tests.

The k-nearest-neighbour indices of SconeOcc are taken from the HIP forward (the selection is piecewise constant: no gradient
flows through it, exactly as with torch.topk indices in the reference, utils.py:1505-1509).
"""
import math
import os

import torch
import torch.nn.functional as F


# ---- real spherical harmonics of a direction, Cartesian form (polar axis +Y, azimuth from +Z toward +X, Condon-Shortley;
# channel k = l*l + l + m: spherical_harmonics.py:111-157 with CustomGeometry.py:27-45 folded in) --------------------------------
def sh_basis(n, max_rank=8):
    """n [..., 3] unit vectors -> [..., max_rank^2].  Y_l^m = N_lm (-1)^m Q_l^m(n_y) {Re, Im}[(n_z + i n_x)^m] where
    P_l^m(x) = (-1)^m (1 - x^2)^(m/2) Q_l^m(x): polynomials only, differentiable everywhere (also on the +-Y axis)."""
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    re, im = [torch.ones_like(ny)], [torch.zeros_like(ny)]             # (n_z + i n_x)^m = sin^m(polar) e^{i m azimuth}
    for m in range(1, max_rank):
        r_prev, i_prev = re[-1], im[-1]
        re.append(r_prev * nz - i_prev * nx)
        im.append(i_prev * nz + r_prev * nx)
    out = [None] * (max_rank * max_rank)
    for m in range(max_rank):
        dfact = 1.0
        for v in range(2 * m - 1, 1, -2):
            dfact *= v
        q_prev2, q_prev = None, torch.full_like(ny, dfact)              # Q_m^m = (2m-1)!!
        for l in range(m, max_rank):
            if l == m:
                q = q_prev
            elif l == m + 1:
                q = (2 * m + 1) * ny * q_prev
            else:
                q = ((2 * l - 1) * ny * q_prev - (l + m - 1) * q_prev2) / (l - m)
            if l > m:
                q_prev2, q_prev = q_prev, q
            norm = math.sqrt((2 * l + 1) / (4 * math.pi))
            if m == 0:
                out[l * l + l] = norm * q
            else:
                norm *= math.sqrt(2.0 * math.factorial(l - m) / math.factorial(l + m)) * (-1) ** m
                out[l * l + l + m] = norm * q * re[m]
                out[l * l + l - m] = norm * q * im[m]
    return torch.stack(out, dim=-1)


def visibilities(pts, harmonics, X_cam, use_sigmoid=True):
    """[B,C,N]: SconeVis.compute_visibilities (SconeVis.py:164-208) in differentiable torch ops."""
    rays = X_cam[:, :, None, :] - pts[:, None, :, :3]
    n = rays / torch.linalg.norm(rays, dim=-1, keepdim=True)
    z = (sh_basis(n) * harmonics[:, None, :, :]).sum(-1)
    return torch.sigmoid(z) if use_sigmoid else torch.relu(z)


def coverage_gain(pts, harmonics, X_cam, use_sigmoid=True):
    """[B,C]: SconeVis.compute_coverage_gain (SconeVis.py:210-252)."""
    return visibilities(pts, harmonics, X_cam, use_sigmoid).mean(dim=-1)


def macarons_gain(vis_u, world_u, inverse, n_unique, cam_world, volume, distance_th, smooth=False):
    """[K]: the MACARONS-regime gain (macarons_utils.py:1668-1704, ops.macarons_gain_indexed) in differentiable torch ops, in the dtype of
    its inputs: gains[k] = mean_s vis_u[k, inverse[k,s]] * factor(|world_u[k, inverse[k,s]] - cam_world[k]|) * volume[k], 0 where
    n_unique[k] == 0.  vis_u [K,S], world_u [K,S,>=3], inverse int64 [K,S], n_unique [K], cam_world [K,3], volume [K].  inverse None and
    n_unique None: the identity map, every camera non-empty (ops.macarons_gain_).  factor: min(1, (th / d)^2), or with smooth
    1 / (1 + (d / th)^2)."""
    vis, world = vis_u, world_u[..., :3]
    if inverse is not None:
        vis = torch.gather(vis_u, 1, inverse)
        world = torch.gather(world, 1, inverse[..., None].expand(-1, -1, 3))
    d = torch.linalg.norm(world - cam_world[:, None, :], dim=-1)
    if smooth:
        f = 1.0 / (1.0 + (d / distance_th) ** 2)
    else:
        f = (distance_th / d.clamp(min=distance_th)) ** 2
    gains = (vis * f).mean(dim=1) * volume
    return gains if n_unique is None else torch.where(n_unique > 0, gains, torch.zeros_like(gains))


# ---- the networks --------------------------------------------------------------------------------------------------------------
def _lin(x, layer):
    return F.linear(x, layer.weight, layer.bias)


def embedding(emb, x, lengths=None):
    """Attention.py:98-128 (k_for_knn = 0): linear-GELU-linear, optional cloud-wide max, optional raw input."""
    res = _lin(F.gelu(_lin(x, emb.linear1)), emb.linear2)
    parts = [res]
    if emb.global_feature:
        r = res
        if lengths is not None:                     # padded batch: the maximum runs over each cloud's own rows
            valid = torch.arange(x.shape[1], device=x.device)[None, :, None] < lengths.view(-1, 1, 1)
            r = torch.where(valid, res, torch.full_like(res, float("-inf")))
        parts.append(r.max(dim=1, keepdim=True)[0].expand_as(res))
    if emb.concatenate_input:
        parts.append(x)
    return torch.cat(parts, dim=-1)


def encoder(enc, x, lengths=None):
    """Attention.py:278-300: pre-LN multi-head self-attention + residual, pre-LN feed-forward + residual."""
    E, H = enc.embedding_dim, enc.n_heads
    h = F.layer_norm(x, (E,), enc.norm1.weight, enc.norm1.bias)
    B, L = h.shape[0], h.shape[1]
    q = _lin(h, enc.mhsa.w_q).view(B, L, H, -1).transpose(1, 2)
    k = _lin(h, enc.mhsa.w_k).view(B, L, H, -1).transpose(1, 2)
    v = _lin(h, enc.mhsa.w_v).view(B, L, H, -1).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if lengths is not None:
        s = s.masked_fill(torch.arange(L, device=x.device)[None, None, None, :] >= lengths.view(-1, 1, 1, 1), float("-inf"))
    att = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, E)
    x = x + (_lin(att, enc.mhsa.out) if H > 1 else att)
    if enc.FF:
        h = F.layer_norm(x, (E,), enc.norm2.weight, enc.norm2.bias)
        x = x + _lin(F.gelu(_lin(h, enc.ff.linear1)), enc.ff.linear2)
    return x


def scone_vis(model, pts, view_harmonics, lengths=None):
    """SconeVis.forward (SconeVis.py:121-162), default architecture."""
    if lengths is not None:                         # the kernels treat an empty cloud as its first row (max(1, length)); so does this
        lengths = lengths.clamp(min=1)
    x = embedding(model.embedding, pts, lengths)
    for enc in model.encoders:
        x = encoder(enc, x, lengths)
    x = F.layer_norm(x, (x.shape[-1],), model.norm.weight, model.norm.bias)
    x = F.gelu(_lin(x, model.fc1))
    x = F.gelu(_lin(torch.cat((x, view_harmonics), dim=-1), model.fc2))
    return _lin(x, model.fc3)


def pc_transformer(pct, x):
    """PCTransformer.forward (SconeOcc.py:104-130): [S,L,3] -> [S, feature_dim] = max || mean over the sequence."""
    x = embedding(pct.embedding, x)
    for enc in pct.encoders:
        x = encoder(enc, x)
    x = _lin(F.layer_norm(x, (x.shape[-1],), pct.norm.weight, pct.norm.bias), pct.linear0)
    return torch.cat((x.max(dim=1)[0], x.mean(dim=1)), dim=-1)


def _env_mode(value, allowed, default):
    """`value` (what the environment holds for a *_BWD variable; read at the call, where the name stands next to os.environ for the scan of
    tests/test_knobs_cpu.py) lower-cased if it is one of `allowed`, else `default`."""
    mode = value.lower()
    return mode if mode in allowed else default


def scone_occ_backward_mode():
    """'composite' (default), 'pct' (env MCR_SCONE_OCC_BWD=pct: the four PCTransformers of the recomputation on the HIP backward) or
    'hip' (MCR_SCONE_OCC_BWD=hip: the whole network's backward behind one entry, SconeOccFunction; with a gradient wanted for the surface
    points, the 'pct' route).  Anything else: 'composite'."""
    return _env_mode(os.environ.get("MCR_SCONE_OCC_BWD", ""), ("pct", "hip"), "composite")


def scone_occ(model, pc_global, scales, x, view_harmonics, knn_idx):
    """SconeOcc.forward (SconeOcc.py:250-347) given the down-sampled clouds and, per scale, the neighbour indices [B,Q,16]."""
    if scone_occ_backward_mode() in ("pct", "hip"):  # the module's own forward: PCTransformerFunction where a gradient is needed
        return _scone_occ(lambda pct, pc: pct(pc), model, pc_global, scales, x, view_harmonics, knn_idx)
    return _scone_occ(pc_transformer, model, pc_global, scales, x, view_harmonics, knn_idx)


def _scone_occ(pc_transformer, model, pc_global, scales, x, view_harmonics, knn_idx):
    B, Q = x.shape[0], x.shape[1]
    feats = [pc_transformer(model.global_transformer, pc_global)[:, None, :].expand(-1, Q, -1)]
    for pc_s, idx, lt in zip(scales, knn_idx, model.local_transformers):
        nb = torch.gather(pc_s[:, None].expand(-1, Q, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3))      # [B,Q,16,3]
        off = nb - x[:, :, None, :]
        feats.append(pc_transformer(lt, off.reshape(B * Q, idx.shape[-1], 3)).view(B, Q, -1))
    xe = model.x_embedding
    feats.append(F.gelu(_lin(F.gelu(_lin(F.gelu(_lin(x, xe.linear1)), xe.linear2)), xe.linear3)))
    feats.append(view_harmonics)
    h = torch.cat(feats, dim=-1)
    return F.gelu(_lin(F.gelu(_lin(F.gelu(_lin(h, model.linear1)), model.linear2)), model.linear3))


def scone_occ_ragged(model, pc_global, global_len, offsets, x, view_harmonics, row_job):
    """The ragged occupancy pass (SconeOcc.forward_ragged: J forward() calls of different sizes) as one differentiable torch composite,
    in the dtype of its inputs: pc_global [J,Lg,3] padded sequences of global_len [J] valid rows (clamped to [1, Lg]), offsets per scale
    [T,16,3] (neighbour minus query), x [T,3], view_harmonics [T,64], row_job [T] -> [T,1].  The global transformer masks the padded
    keys and pools over each sequence's valid rows (max; mean divided by their number); the padding rows are never read (they are
    replaced by the sequence's first row before anything else).  The neighbourhoods have the value of `offsets` and gradient -1
    towards x; the selection and the clouds carry none."""
    J, Lg = pc_global.shape[0], pc_global.shape[1]
    n = global_len.to(pc_global.device).long().clamp(1, Lg)
    valid = torch.arange(Lg, device=pc_global.device)[None, :, None] < n.view(-1, 1, 1)
    t = model.global_transformer
    h = embedding(t.embedding, torch.where(valid, pc_global.detach(), pc_global.detach()[:, :1]))
    for enc in t.encoders:
        h = encoder(enc, h, n)
    h = _lin(F.layer_norm(h, (h.shape[-1],), t.norm.weight, t.norm.bias), t.linear0)
    g_max = torch.where(valid, h, torch.full_like(h, float("-inf"))).max(dim=1)[0]
    g_avg = torch.where(valid, h, torch.zeros_like(h)).sum(dim=1) / n[:, None].to(h.dtype)
    feats = [torch.cat((g_max, g_avg), dim=-1)[row_job.long()]]
    to_x = (x.detach() - x)[:, None, :]
    for off, lt in zip(offsets, model.local_transformers):
        feats.append(pc_transformer(lt, off.detach() + to_x))
    xe = model.x_embedding
    feats.append(F.gelu(_lin(F.gelu(_lin(F.gelu(_lin(x, xe.linear1)), xe.linear2)), xe.linear3)))
    feats.append(view_harmonics)
    h = torch.cat(feats, dim=-1)
    return F.gelu(_lin(F.gelu(_lin(F.gelu(_lin(h, model.linear1)), model.linear2)), model.linear3))


# ---- HIP forward + composite backward --------------------------------------------------------------------------------------
class _HipForwardTorchBackward(torch.autograd.Function):
    """apply(hip_fn, torch_fn, n_tensor_inputs, *tensor_inputs_then_params): forward = hip_fn(*inputs) without a graph;
    backward = autograd through torch_fn(*inputs) (recomputed) for every input / parameter that requires a gradient."""

    @staticmethod
    def forward(ctx, hip_fn, torch_fn, n_in, *tensors):
        ctx.torch_fn, ctx.n_in = torch_fn, n_in
        ctx.inputs = tensors[:n_in]                 # plain references: nothing but the op's own inputs is kept for the backward
        ctx.params = tensors[n_in:]
        with torch.no_grad():
            return hip_fn(*tensors[:n_in])

    @staticmethod
    def backward(ctx, grad_out):
        n_in = ctx.n_in
        with torch.enable_grad():
            ins = [t.detach().requires_grad_(True) if (t.is_floating_point() and ctx.needs_input_grad[3 + i]) else t
                   for i, t in enumerate(ctx.inputs)]
            out = ctx.torch_fn(*ins)                # the composite reads the module's own parameters
            wrt = [(i, t) for i, t in enumerate(ins) if t.requires_grad and ctx.needs_input_grad[3 + i]]
            wrt += [(n_in + j, p) for j, p in enumerate(ctx.params) if ctx.needs_input_grad[3 + n_in + j]]
            grads = torch.autograd.grad(out, [t for _, t in wrt], grad_out, allow_unused=True) if wrt else []
        res = [None] * (n_in + len(ctx.params))
        for (i, _), g in zip(wrt, grads):
            res[i] = g
        return (None, None, None, *res)


def needs_grad(module, *tensors):
    return torch.is_grad_enabled() and (any(getattr(t, "requires_grad", False) for t in tensors if t is not None)
                                        or (module is not None and any(p.requires_grad for p in module.parameters())))


def with_torch_backward(hip_fn, torch_fn, inputs, module=None):
    """Run hip_fn(*inputs); if a gradient is needed, make the result differentiable through torch_fn(*inputs)."""
    params = tuple(module.parameters()) if module is not None else ()
    return _HipForwardTorchBackward.apply(hip_fn, torch_fn, len(inputs), *inputs, *params)


# ---- what the HIP-backward Functions share ---------------------------------------------------------------------------------------
def _once(what, why="its HIP backward builds no graph"):
    """The guard of every Function below: `what` (subject and verb, 'the cost volume is') can be differentiated once."""
    if torch.is_grad_enabled():
        raise RuntimeError(f"{what} differentiable once: {why} (create_graph is not supported)")


def _slot_grads(ctx, d_w, first, dtypes=None):
    """The gradients of a network Function's parameters from the weight-gradient table d_w: ctx.slots[j] = (table index, row slice or
    None) of parameter j, whose needs_input_grad is number first + j; None where no gradient is needed.  dtypes: cast to dtypes[j]."""
    grads = []
    for j, (i, rows) in enumerate(ctx.slots):
        if not ctx.needs_input_grad[first + j]:
            grads.append(None)
            continue
        g = d_w[i] if rows is None else d_w[i][rows[0]:rows[1]]
        grads.append(g if dtypes is None else g.to(dtypes[j]))
    return grads


# ---- SconeVis: HIP forward + HIP backward ----------------------------------------------------------------------------------------
def scone_vis_backward_mode():
    """'hip' (default) or 'composite' (env MCR_SCONE_VIS_BWD=composite: the recomputing torch backward above, for A/B comparisons)."""
    return _env_mode(os.environ.get("MCR_SCONE_VIS_BWD", ""), ("composite",), "hip")


class SconeVisFunction(torch.autograd.Function):
    """apply(hip_fn, table_fn, slots, lengths, pts, view_harmonics, *params): forward = hip_fn(pts, view_harmonics) without a graph;
    backward = ops.scone_vis_backward (mcr_scone_vis_backward: the gradient of the fp32 network, HIP kernels only) on the weight
    table table_fn() returns.  slots[j] = (table index, row slice or None) of params[j] -- the packed qkv entries hand rows 0:64,
    64:128 and 128:384 to w_q, w_k and w_v.  Differentiable once."""

    @staticmethod
    def forward(ctx, hip_fn, table_fn, slots, lengths, pts, view_harmonics, *params):
        ctx.table_fn, ctx.slots, ctx.lengths = table_fn, slots, lengths
        ctx.save_for_backward(pts, view_harmonics)
        with torch.no_grad():
            return hip_fn(pts, view_harmonics)

    @staticmethod
    def backward(ctx, grad_out):
        _once("SconeVis.forward is")
        from . import ops
        pts, vh = ctx.saved_tensors
        need_p, need_v = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        need_w = any(ctx.needs_input_grad[6:])
        d_w, d_pts, d_vh = ops.scone_vis_backward(pts, vh, grad_out, ctx.table_fn(), ctx.lengths, need=(need_w, need_p, need_v))
        # NOT cast to the parameters' dtypes, unlike the three Functions below: SconeVis hands out the table's fp32 gradients as they are
        return (None, None, None, None, d_pts.to(pts.dtype) if d_pts is not None else None,
                d_vh.to(vh.dtype) if d_vh is not None else None, *_slot_grads(ctx, d_w, 6))


# ---- PCTransformer: HIP forward + HIP backward -----------------------------------------------------------------------------------
class PCTransformerFunction(torch.autograd.Function):
    """apply(hip_fn, table_fn, slots, feature_dim, pc, *params): forward = hip_fn(pc) without a graph; backward =
    ops.pc_transformer_backward (mcr_pc_transformer_backward: the gradient of the fp32 network, HIP kernels only) on the weight table
    table_fn() returns.  slots[j] = (table index, row slice or None) of params[j] -- the packed qkv entries hand rows 0:32, 32:64 and
    64:192 to w_q, w_k and w_v.  Differentiable once."""

    @staticmethod
    def forward(ctx, hip_fn, table_fn, slots, feature_dim, pc, *params):
        ctx.table_fn, ctx.slots, ctx.feature_dim = table_fn, slots, feature_dim
        ctx.param_dtypes = tuple(p.dtype for p in params)
        ctx.save_for_backward(pc)
        with torch.no_grad():
            return hip_fn(pc)

    @staticmethod
    def backward(ctx, grad_out):
        _once("PCTransformer.forward is")
        from . import ops
        pc, = ctx.saved_tensors
        need_p, need_w = ctx.needs_input_grad[4], any(ctx.needs_input_grad[5:])
        d_w, d_pc = ops.pc_transformer_backward(pc, grad_out, ctx.table_fn(), ctx.feature_dim, need=(need_w, need_p))
        return (None, None, None, None, d_pc.to(pc.dtype) if d_pc is not None else None, *_slot_grads(ctx, d_w, 5, ctx.param_dtypes))


# ---- SconeOcc: HIP forward + HIP backward ----------------------------------------------------------------------------------------
class SconeOccFunction(torch.autograd.Function):
    """apply(hip_fn, table_fn, slots, k, pc_global, scales, x, view_harmonics, *params): forward = hip_fn(pc_global, scales, x,
    view_harmonics) without a graph; backward = ops.scone_occ_backward (mcr_scone_occ_backward: the gradient of the fp32 network, HIP
    kernels only) on the weight table table_fn() returns, with the k neighbour indices of every scale taken by ops.knn_points on the
    detached inputs, as the composite route takes them.  slots[j] = (table index, row slice or None) of params[j] -- the packed qkv
    entries of the four transformers hand rows 0:32, 32:64 and 64:192 to w_q, w_k and w_v.  The clouds (pc_global, the list `scales`)
    get no gradient.  Differentiable once."""

    @staticmethod
    def forward(ctx, hip_fn, table_fn, slots, k, pc_global, scales, x, view_harmonics, *params):
        ctx.table_fn, ctx.slots, ctx.k = table_fn, slots, k
        ctx.param_dtypes = tuple(p.dtype for p in params)
        ctx.save_for_backward(pc_global, x, view_harmonics, *scales)
        with torch.no_grad():
            return hip_fn(pc_global, scales, x, view_harmonics)

    @staticmethod
    def backward(ctx, grad_out):
        _once("SconeOcc.forward is")
        from . import ops
        pc_global, x, vh, *scales = ctx.saved_tensors
        need_x, need_v = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        need_w = any(ctx.needs_input_grad[8:])
        xq = x.detach().float().contiguous()
        sc = [s_.detach().float().contiguous() for s_ in scales]
        idx = [ops.knn_points(xq, s_, ctx.k)[2] for s_ in sc]
        d_w, d_x, d_vh = ops.scone_occ_backward(pc_global.detach().float(), sc, xq, vh.detach().float(), idx, grad_out.float(),
                                                ctx.table_fn(), need=(need_w, need_x, need_v))
        return (None, None, None, None, None, None, d_x.to(x.dtype) if d_x is not None else None,
                d_vh.to(vh.dtype) if d_vh is not None else None, *_slot_grads(ctx, d_w, 8, ctx.param_dtypes))


class SconeOccRaggedFunction(torch.autograd.Function):
    """apply(hip_fn, table_fn, slots, scale_sizes, query_sizes, pc_global, global_len, clouds, row_job, x, view_harmonics, *params):
    forward = hip_fn() (the ragged HIP forward on these very tensors) without a graph; backward = the three scales' neighbourhood
    offsets by ops.knn_offsets_segmented on the detached inputs (clouds[i]: the jobs' scale-i clouds one behind the other,
    scale_sizes[i]: their sizes), then ONE ops.scone_occ_backward_ragged (mcr_scone_occ_backward_ragged: the gradient of the fp32
    network, HIP kernels only, weight gradients summed over the jobs).  slots as SconeOccFunction.  The clouds get no gradient.
    Differentiable once."""

    @staticmethod
    def forward(ctx, hip_fn, table_fn, slots, scale_sizes, query_sizes, pc_global, global_len, clouds, row_job, x, view_harmonics, *params):
        ctx.table_fn, ctx.slots, ctx.scale_sizes, ctx.query_sizes = table_fn, slots, scale_sizes, [int(q) for q in query_sizes]
        ctx.param_dtypes = tuple(p.dtype for p in params)
        ctx.save_for_backward(pc_global, global_len, row_job, x, view_harmonics, *clouds)
        with torch.no_grad():
            return hip_fn()

    @staticmethod
    def backward(ctx, grad_out):
        _once("SconeOcc.forward_ragged is")
        from . import ops
        pc_global, global_len, row_job, x, vh, *clouds = ctx.saved_tensors
        need_x, need_v = ctx.needs_input_grad[9], ctx.needs_input_grad[10]
        need_w = any(ctx.needs_input_grad[11:])
        xq = x.detach().float().contiguous()
        offsets = [ops.knn_offsets_segmented(xq, c_.detach().float().contiguous(), sizes, ctx.query_sizes)
                   for c_, sizes in zip(clouds, ctx.scale_sizes)]
        d_w, d_x, d_vh = ops.scone_occ_backward_ragged(pc_global.detach().float(), global_len, offsets, xq, vh.detach().float(), row_job,
                                                       ctx.query_sizes, grad_out.float(), ctx.table_fn(), need=(need_w, need_x, need_v))
        return (None,) * 9 + (d_x.to(x.dtype) if d_x is not None else None, d_vh.to(vh.dtype) if d_vh is not None else None,
                              *_slot_grads(ctx, d_w, 11, ctx.param_dtypes))


# ---- MACARONS-regime gain: HIP forward + HIP backward ----------------------------------------------------------------------------
class MacaronsGainFunction(torch.autograd.Function):
    """apply(vis, world, inverse, n_unique, cam_world, volume, distance_th, smooth) -> gains [K]: forward = ops.macarons_gain_indexed
    without a graph (inverse and n_unique None, the identity form: ops.macarons_gain_ on a private copy of vis, which it scales in
    place) -- the values keep the bits of those calls; backward = one ops.macarons_gain_backward (mcr_macarons_gain_backward).
    Gradients go to vis and, if it requires one, to volume; world, inverse, n_unique and cam_world are constants of the graph.
    Differentiable once."""

    @staticmethod
    def forward(ctx, vis, world, inverse, n_unique, cam_world, volume, distance_th, smooth):
        from . import ops
        ctx.distance_th, ctx.smooth = float(distance_th), bool(smooth)
        ctx.save_for_backward(vis, world, inverse, n_unique, cam_world, volume)
        with torch.no_grad():
            if inverse is None and n_unique is None:
                return ops.macarons_gain_(vis.clone(), world, cam_world, volume, distance_th, smooth)
            return ops.macarons_gain_indexed(vis, world, inverse, n_unique, cam_world, volume, distance_th, smooth)

    @staticmethod
    def backward(ctx, grad_gains):
        _once("the MACARONS gain is")
        from . import ops
        vis, world, inverse, n_unique, cam_world, volume = ctx.saved_tensors
        d_vis, d_volume = ops.macarons_gain_backward(grad_gains.float().contiguous(), vis, world, inverse, n_unique, cam_world, volume,
                                                     ctx.distance_th, ctx.smooth, need_volume=ctx.needs_input_grad[5])
        return (d_vis if ctx.needs_input_grad[0] else None, None, None, None, None, d_volume, None, None)


# ---- occupancy supervision pass: scatter into upstream's return value, HIP forward + HIP backward --------------------------------
class SupervisionScatterFunction(torch.autograd.Function):
    """apply(occ, rows, job_offsets, n_jobs, pos, n_out) -> [n_out,1]: forward = ops.supervision_scatter (mcr_supervision_scatter: the rows
    of the first n_jobs jobs of occ [T,1] added in job order to zeros, the `proxy_probas[cell_X_mask] += cell_occ_probs` of
    macarons_utils.py:1371 read at prediction_mask) without a graph; backward = ops.supervision_scatter_backward (an exact gather; the
    rows behind the scattered jobs -- the dummy passes' -- receive zeros, so that every parameter behind occ gets a gradient tensor).
    Differentiable once."""

    @staticmethod
    def forward(ctx, occ, rows, job_offsets, n_jobs, pos, n_out):
        from . import ops
        ctx.T, ctx.n_jobs = occ.shape[0], int(n_jobs)
        ctx.T_scatter = 0 if rows is None else int(rows.numel())
        ctx.save_for_backward(rows, pos)
        with torch.no_grad():
            return ops.supervision_scatter(rows, occ.detach().float().reshape(-1), job_offsets, ctx.n_jobs if ctx.T_scatter else 0, pos, int(n_out))

    @staticmethod
    def backward(ctx, grad_out):
        _once("the supervision scatter is")
        from . import ops
        rows, pos = ctx.saved_tensors
        d_occ = ops.supervision_scatter_backward(rows, pos, grad_out.float().contiguous(), ctx.T_scatter if ctx.n_jobs else 0, ctx.T)
        return d_occ, None, None, None, None, None


# ---- depth module, the plane sweep: HIP forward + HIP backward --------------------------------------------------------------------
def cost_volume_backward_mode():
    """'hip' (default) or 'composite' (env MCR_COST_VOLUME_BWD=composite: the recomputing torch backward, for A/B comparisons)."""
    return _env_mode(os.environ.get("MCR_COST_VOLUME_BWD", ""), ("composite",), "hip")


class CostVolumeFunction(torch.autograd.Function):
    """apply(x, x_alpha, cams, depth_bins, H, W, fov_scale, concat) -> the cost volume [B,D,Hf,Wf] of ops.cost_volume (mcr_cost_volume)
    without a graph, or with concat the buffer [B,C+D,Hf,Wf] = cat(x, cost volume) of ManyDepth.py:299, the volume written in place
    by the kernel.  backward = ops.cost_volume_backward (mcr_cost_volume_backward, cost_volume_bwd.hip: no floating-point atomics, the
    same bits on every run) for x and x_alpha, each computed only if its input needs it; the cameras and the bins are constants of
    the graph.  With cost_volume_backward_mode() == 'composite' the backward is autograd through networks.ManyDepth.cost_volume_planes
    instead (plain torch on the same device, recomputed PLANE_CHUNK planes at a time so that its intermediates stay bounded).
    Differentiable once."""

    PLANE_CHUNK = 8

    @staticmethod
    def forward(ctx, x, x_alpha, cams, depth_bins, H, W, fov_scale, concat):
        from . import ops
        ctx.H, ctx.W, ctx.fov_scale, ctx.concat = int(H), int(W), float(fov_scale), bool(concat)
        ctx.save_for_backward(x, x_alpha, cams, depth_bins)
        with torch.no_grad():
            if not concat:
                return ops.cost_volume(x, x_alpha, cams, depth_bins, H, W, fov_scale)
            B, C, Hf, Wf = x.shape
            buf = torch.empty((B, C + depth_bins.numel(), Hf, Wf), dtype=torch.float32, device=x.device)
            buf[:, :C].copy_(x)
            ops.cost_volume(x, x_alpha, cams, depth_bins, H, W, fov_scale, out=buf[:, C:])
            return buf

    @staticmethod
    def backward(ctx, grad_out):
        _once("the cost volume is", "its backward recomputes without a graph")
        x, x_alpha, cams, depth_bins = ctx.saved_tensors
        C = x.shape[1]
        g_cv = grad_out[:, C:] if ctx.concat else grad_out
        need = ctx.needs_input_grad[:2]
        if cost_volume_backward_mode() == "hip":
            from . import ops
            d_x, d_xa = (None, None) if not any(need) else ops.cost_volume_backward(
                x, x_alpha, cams, depth_bins, g_cv.float(), ctx.H, ctx.W, ctx.fov_scale, need_x=need[0], need_x_alpha=need[1])
            if ctx.concat and need[0]:
                d_x += grad_out[:, :C]
            return (d_x, d_xa, None, None, None, None, None, None)
        from .networks.ManyDepth import cost_volume_planes
        grads = [None, None]
        with torch.enable_grad():
            ins = [t.detach().requires_grad_(n) for t, n in zip((x, x_alpha), need)]
            wrt = [i for i in (0, 1) if need[i]]
            for k in range(0, depth_bins.numel(), CostVolumeFunction.PLANE_CHUNK) if wrt else ():
                sl = slice(k, k + CostVolumeFunction.PLANE_CHUNK)
                cv = cost_volume_planes(ins[0], ins[1], cams, depth_bins[sl], ctx.H, ctx.W, ctx.fov_scale)
                for i, g in zip(wrt, torch.autograd.grad(cv, [ins[i] for i in wrt], g_cv[:, sl])):
                    grads[i] = g if grads[i] is None else grads[i] + g
        if ctx.concat and need[0]:
            grads[0] = grads[0] + grad_out[:, :C]
        return (grads[0], grads[1], None, None, None, None, None, None)


# ---- depth module, the photometric reconstruction loss: HIP forward + HIP backward --------------------------------------------------
def reconstruction_loss_backward_mode():
    """'hip' (default) or 'composite' (env MCR_RECONSTRUCTION_LOSS_BWD=composite: the recomputing torch backward, for A/B comparisons)."""
    return _env_mode(os.environ.get("MCR_RECONSTRUCTION_LOSS_BWD", ""), ("composite",), "hip")


class ReconstructionLossFunction(torch.autograd.Function):
    """apply(depth, images, alpha_images, mask, cams, zfar, ssim_factor, padding_mode, fov_scale) -> loss [S] of ops.reconstruction_loss
    (mcr_reconstruction_loss).  backward = ops.reconstruction_loss_backward (mcr_reconstruction_loss_backward: a gather per pixel, no
    atomics, the same bits on every run) for depth [S,B,H,W] and for nothing else: the images, the mask and the cameras are constants of
    the graph.  With reconstruction_loss_backward_mode() == 'composite' the backward is autograd through
    networks.ManyDepth.reconstruction_loss_composite instead (plain torch on the same device).  Differentiable once."""

    @staticmethod
    def forward(ctx, depth, images, alpha_images, mask, cams, zfar, ssim_factor, padding_mode, fov_scale):
        from . import ops
        ctx.zfar, ctx.ssim_factor, ctx.padding_mode, ctx.fov_scale = float(zfar), float(ssim_factor), padding_mode, float(fov_scale)
        ctx.has_mask = mask is not None
        ctx.save_for_backward(depth, images, alpha_images, cams, *((mask,) if mask is not None else ()))
        with torch.no_grad():
            return ops.reconstruction_loss(images, alpha_images, mask, cams, depth, zfar, ssim_factor, padding_mode, fov_scale)

    @staticmethod
    def backward(ctx, grad_loss):
        _once("the reconstruction loss is", "its backward recomputes without a graph")
        depth, images, alpha_images, cams = ctx.saved_tensors[:4]
        mask = ctx.saved_tensors[4] if ctx.has_mask else None
        none = (None,) * 8
        if not ctx.needs_input_grad[0]:
            return (None,) + none
        if reconstruction_loss_backward_mode() == "hip":
            from . import ops
            return (ops.reconstruction_loss_backward(images, alpha_images, mask, cams, depth, grad_loss.float().contiguous(), ctx.zfar,
                                                     ctx.ssim_factor, ctx.padding_mode, ctx.fov_scale),) + none
        from .networks.ManyDepth import reconstruction_loss_composite
        with torch.enable_grad():
            d = depth.detach().requires_grad_(True)
            loss = reconstruction_loss_composite(images, alpha_images, mask, cams, d, ctx.zfar, ctx.ssim_factor, ctx.padding_mode, ctx.fov_scale)
            return tuple(torch.autograd.grad(loss, (d,), grad_loss)) + none


# ---- depth module, disparity scales / regularity values / error mask: HIP forward + HIP backward ---------------------------------------
def disparity_scales_backward_mode():
    """'hip' (default) or 'composite' (env MCR_DISPARITY_SCALES_BWD=composite: the recomputing torch backward, for A/B comparisons)."""
    return _env_mode(os.environ.get("MCR_DISPARITY_SCALES_BWD", ""), ("composite",), "hip")


class DisparityScalesFunction(torch.autograd.Function):
    """apply(images, mask, znear, zfar, *disps) -> (depth [S,B,H,W], reg [S], error_mask [B,H,W] bool) of ops.disparity_scales
    (mcr_disparity_scales).  Differentiable in the disparities only, through depth and reg; error_mask is marked non-differentiable.
    backward = ops.disparity_scales_backward (mcr_disparity_scales_backward: no atomics, the same bits on every run); a half whose
    gradient is absent or not needed is not computed.  With disparity_scales_backward_mode() == 'composite' the backward is autograd
    through networks.ManyDepth.disparity_scales_composite instead (plain torch on the same device).  Differentiable once."""

    @staticmethod
    def forward(ctx, images, mask, znear, zfar, *disps):
        from . import ops
        ctx.znear, ctx.zfar, ctx.has_mask = float(znear), float(zfar), mask is not None
        ctx.save_for_backward(images, *((mask,) if mask is not None else ()), *disps)
        with torch.no_grad():
            depth, reg, error_mask = ops.disparity_scales(disps, images, mask, znear, zfar)
        ctx.mark_non_differentiable(error_mask)
        ctx.set_materialize_grads(False)
        return depth, reg, error_mask

    @staticmethod
    def backward(ctx, grad_depth, grad_reg, _grad_error_mask):
        _once("the disparity scales are", "their backward recomputes without a graph")
        images = ctx.saved_tensors[0]
        mask = ctx.saved_tensors[1] if ctx.has_mask else None
        disps = ctx.saved_tensors[2 if ctx.has_mask else 1:]
        none = (None,) * 4
        if not any(ctx.needs_input_grad[4:]) or (grad_depth is None and grad_reg is None):
            return none + (None,) * len(disps)
        if disparity_scales_backward_mode() == "hip":
            from . import ops
            grads = ops.disparity_scales_backward(disps, images, mask, ctx.znear, ctx.zfar,
                                                  None if grad_depth is None else grad_depth.float().contiguous(),
                                                  None if grad_reg is None else grad_reg.float().contiguous())
            return none + tuple(g.reshape(d.shape) if n else None for g, d, n in zip(grads, disps, ctx.needs_input_grad[4:]))
        from .networks.ManyDepth import disparity_scales_composite
        with torch.enable_grad():
            leaves = [d.detach().requires_grad_(True) for d in disps]
            depth, reg, _ = disparity_scales_composite(leaves, images, mask, ctx.znear, ctx.zfar)
            outs, gouts = zip(*[(o, g) for o, g in ((depth, grad_depth), (reg, grad_reg)) if g is not None])
            grads = torch.autograd.grad(outs, leaves, gouts)
        return none + tuple(g if n else None for g, n in zip(grads, ctx.needs_input_grad[4:]))


# ---- depth module, the disparity heads: HIP forward + HIP backward -------------------------------------------------------------------------
def disparity_head_backward_mode():
    """'composite' (default) or 'hip' (env MCR_DISPARITY_HEAD_BWD=hip: the HIP backward mcr_disparity_head_backward).  The default is the
    torch composite because profiles/disparity_head_times.json does not show a forward-and-backward step through the Function faster
    with the intervals apart at every shape (nine rows of ten; not at [4,128,32,57]): a step of one head is bound by the host either
    way, not by the kernels (NOTES.md)."""
    return _env_mode(os.environ.get("MCR_DISPARITY_HEAD_BWD", ""), ("hip",), "composite")


class DisparityHeadFunction(torch.autograd.Function):
    """apply(x, weight, bias) -> y [B,1,Hs,Ws] of ops.disparity_head (mcr_disparity_head): x [B,C,Hs,Ws], weight [1,C,3,3], bias [1].
    Saves x, weight and y (and the bias, which only the composite route reads).  backward = ops.disparity_head_backward (mcr_disparity_head_backward: no atomics, the same bits on every
    run) with disparity_head_backward_mode() == 'hip'; the d_x half and the d_weight / d_bias half each run only if an input needs them.
    With the mode 'composite' (the default) the backward is autograd through networks.ManyDepth.disparity_head_composite instead (plain
    torch on the same device, recomputed; for A/B runs -- the module's forward does not come here in that mode, it runs the composite
    under autograd directly).  Differentiable once."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import ops
        with torch.no_grad():
            y = ops.disparity_head(x, weight, bias)
        ctx.save_for_backward(x, weight, bias, y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        _once("the disparity head is", "its backward runs without a graph")
        x, weight, bias, y = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad)
        if not any(need):
            return None, None, None
        if disparity_head_backward_mode() == "hip":
            from . import ops
            return ops.disparity_head_backward(x, weight, y, grad_y.float().contiguous(), need=need)
        from .networks.ManyDepth import disparity_head_composite
        with torch.enable_grad():
            ins = [t.detach().requires_grad_(n) for t, n in zip((x, weight, bias), need)]
            grads = iter(torch.autograd.grad(disparity_head_composite(*ins), [t for t, n in zip(ins, need) if n], grad_y))
        return tuple(next(grads) if n else None for n in need)


# ---- depth module, the expansion layers: HIP forward + HIP backward ------------------------------------------------------------------------
def expansion_layer_backward_mode():
    """'composite' (default) or 'hip' (env MCR_EXPANSION_LAYER_BWD=hip: the fused forward and the HIP backward
    mcr_expansion_layer_backward, through ExpansionLayerFunction).  The default is the torch composite under autograd because
    profiles/expansion_layer_backward_times.json does not show a forward-and-backward step through the Function faster with the
    intervals apart at every shape (seven rows of ten: all five of upstream's shapes at B 1, expansion2 and expansion1 at B 4; not at
    expansion5, expansion4 and expansion3 at B 4, where the library's convolutions are faster than the exact-fp32 kernels), and the
    route stays opt-in whatever that file shows (NOTES.md); the five layers with the four heads, all three knobs on, are faster with
    the intervals apart at both batch sizes."""
    return _env_mode(os.environ.get("MCR_EXPANSION_LAYER_BWD", ""), ("hip",), "composite")


class ExpansionLayerFunction(torch.autograd.Function):
    """apply(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size) -> y [B,Cout,H,W] of ops.expansion_layer (mcr_expansion_layer);
    x_add None: no concatenation.  Saves x, x_add, the weights, u (the transposed convolution after its ELU, which the forward leaves at
    the front of its workspace) and y (and the biases, which only the composite route reads).  backward = ops.expansion_layer_backward
    (mcr_expansion_layer_backward: no atomics, the same bits on every run) with expansion_layer_backward_mode() == 'hip'; a gradient
    that no input needs is not computed, nor a launch that only it depends on.  With the mode 'composite' the backward is autograd
    through networks.ManyDepth.expansion_layer_composite instead (plain torch on the same device, recomputed; for A/B runs -- the
    module's forward does not come here in that mode).  Differentiable once."""

    @staticmethod
    def forward(ctx, x, x_add, up_weight, up_bias, i_weight, i_bias, output_size):
        from . import ops
        ctx.output_size, ctx.has_add = tuple(int(v) for v in output_size), x_add is not None
        with torch.no_grad():
            y, u = ops.expansion_layer(x, x_add, up_weight, up_bias, i_weight, i_bias, ctx.output_size, return_u=True)
        ctx.save_for_backward(x, up_weight, up_bias, i_weight, i_bias, u, y, *((x_add,) if ctx.has_add else ()))
        return y

    @staticmethod
    def backward(ctx, grad_y):
        _once("the expansion layer is", "its backward runs without a graph")
        x, up_weight, up_bias, i_weight, i_bias, u, y = ctx.saved_tensors[:7]
        x_add = ctx.saved_tensors[7] if ctx.has_add else None
        need = tuple(ctx.needs_input_grad[:6])
        if not ctx.has_add:
            need = (need[0], False) + need[2:]
        if not any(need):
            return (None,) * 7
        if expansion_layer_backward_mode() == "hip":
            from . import ops
            return ops.expansion_layer_backward(x, x_add, up_weight, i_weight, u, y, grad_y.float().contiguous(), ctx.output_size,
                                                need=need) + (None,)
        from .networks.ManyDepth import expansion_layer_composite
        with torch.enable_grad():
            ins = [None if t is None else t.detach().requires_grad_(n) for t, n in zip((x, x_add, up_weight, up_bias, i_weight, i_bias), need)]
            grads = iter(torch.autograd.grad(expansion_layer_composite(*ins, ctx.output_size), [t for t, n in zip(ins, need) if n], grad_y))
        return tuple(next(grads) if n else None for n in need) + (None,)
