"""The plane sweep of the depth module on HIP: a mirror of upstream's `CostVolumeBuilder` (macarons/networks/ManyDepth.py:80-305) whose
forward builds the cost volume with one fused entry (ops.cost_volume -> mcr_cost_volume, csrc/cost_volume.hip) instead of upstream's
cameras / unprojection / projection / bicubic resize / 96-fold feature copy / grid_sample / mean / norm sequence, and the seam that puts
an existing upstream instance on that path (`adopt_cost_volume_builder`).  The rest of the depth network -- layers 2-4 of the ResNet
encoder, the pose decoder, `apply_depth_model` -- is convolutions the vendor library serves and stays upstream's.  The photometric
reconstruction loss is fused on HIP as well (ops.reconstruction_loss -> mcr_reconstruction_loss, csrc/reconstruction_loss.hip, behind
utility.macarons_utils.get_reconstruction_loss_fn); `reconstruction_loss_composite` below is the same mathematics in plain
differentiable torch, for the cases the entry does not take and for the tests.  So is the step between the network's disparity maps
and that loss (ops.disparity_scales -> mcr_disparity_scales, csrc/disparity_scales.hip, behind utility.macarons_utils.depth_scale_losses):
`disparity_scales_composite` below is its plain-torch form.  And so are the decoder's four disparity heads, the last link upstream of those
maps (ops.disparity_head -> mcr_disparity_head, csrc/disparity_head.hip): `DisparityLayer` mirrors upstream's class (ManyDepth.py:366-384),
`adopt_disparity_layer` / `adopt_depth_decoder` put existing upstream instances on it, `disparity_head_composite` is its plain-torch form.
What feeds those heads, the decoder's five expansion layers (ManyDepth.py:308-363: a transposed convolution, ELU, a nearest resize, a
concatenation, a reflection-padded convolution, ELU), has a fused forward too (ops.expansion_layer -> mcr_expansion_layer,
csrc/expansion_layer.hip, exact-fp32 matrix instructions): `ExpansionLayer` mirrors the class, `adopt_expansion_layer` and
`adopt_depth_decoder` adopt upstream instances, `expansion_layer_composite` is the plain-torch form and `expansion_layer_route` says which
of the two a forward takes.  The front of the encoder -- the 7 x 7 convolution, BatchNorm, ReLU, the max-pool and the basic blocks of
`layer1`, which the decoder runs on the target and on every source image -- is one entry in eval mode (ops.feature_extractor ->
mcr_feature_extractor, csrc/resnet_stem.hip and csrc/basic_block.hip): `BasicBlock` and `FeatureExtractor` mirror the classes,
`adopt_feature_extractor` and `adopt_depth_front` adopt upstream instances, the `*_composite` functions are the plain-torch forms and
`feature_extractor_route` says which a forward takes.

Needs neither PyTorch3D nor torchvision: a camera is its R, T (PyTorch3D's row-vector convention, view = world @ R + T) and the default
60 degree field of view upstream never overrides; znear and zfar drop out of the sweep (they only shape the z the projection returns,
which upstream discards, and the scaled depth the unprojection immediately inverts).

The backward is HIP as well (ops.cost_volume_backward -> mcr_cost_volume_backward, csrc/cost_volume_bwd.hip, behind CostVolumeFunction).
`cost_volume_composite` is the same mathematics in plain differentiable torch, chunked over the planes: what CostVolumeFunction
differentiates instead under MCR_COST_VOLUME_BWD=composite (autograd.py) and what the tests hold against an independent fp64 model.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from ..ops import COST_VOLUME_FOV_SCALE

__all__ = ["CostVolumeBuilder", "adopt_cost_volume_builder", "DisparityLayer", "adopt_disparity_layer", "ExpansionLayer",
           "adopt_expansion_layer", "adopt_depth_decoder", "BasicBlock", "FeatureExtractor", "adopt_feature_extractor", "adopt_depth_front"]


def pack_cameras(R, T, R_alpha, T_alpha):
    """R [B,3,3], T [B,3], R_alpha [B,A,3,3], T_alpha [B,A,3] -> cams [B,1+A,12] float32 (row 0 the target; R row-major, then T)."""
    B, A = R_alpha.shape[0], R_alpha.shape[1]
    tgt = torch.cat((R.reshape(B, 1, 9), T.reshape(B, 1, 3)), -1)
    src = torch.cat((R_alpha.reshape(B, A, 9), T_alpha.reshape(B, A, 3)), -1)
    return torch.cat((tgt, src), 1).float().contiguous()


def _source_rays(cams, H, W, fov_scale, dtype, device):
    """cams [B,1+A,12] -> (u [B,A,H,W,3], t [B,A,3]): the source-view point of full-resolution pixel (p, q) at depth d is
    d * u[b,a,p,q] + t[b,a], for every source a of image b."""
    B, A = cams.shape[0], cams.shape[1] - 1
    cams = cams.to(dtype)
    R, T = cams[:, 0, :9].reshape(B, 3, 3), cams[:, 0, 9:]
    Ra, Ta = cams[:, 1:, :9].reshape(B, A, 3, 3), cams[:, 1:, 9:]
    m = min(H, W)
    # the ray of full-resolution pixel (p, q) in the target view, per unit depth (reproject_depth_map, ManyDepth.py:128-137)
    nx = (W / m - 2.0 * torch.arange(W, dtype=dtype, device=device) / (m - 1)) / fov_scale
    ny = (H / m - 2.0 * torch.arange(H, dtype=dtype, device=device) / (m - 1)) / fov_scale
    n = torch.stack((nx[None, :].expand(H, W), ny[:, None].expand(H, W), torch.ones(H, W, dtype=dtype, device=device)), -1)
    # target view -> world -> source view is affine: v_a = v (R^T R_a) + (T_a - T R^T R_a), hence affine in the depth along a ray
    M = torch.einsum("bij,baik->bajk", R, Ra)
    u = torch.einsum("hwj,bajk->bahwk", n, M)
    return u, Ta - torch.einsum("bj,bajk->bak", T, M)


def cost_volume_planes(x, x_alpha, cams, depth_bins, H, W, fov_scale=COST_VOLUME_FOV_SCALE):
    """The cost volume [B,len(depth_bins),Hf,Wf] of the given planes in torch ops, in x's dtype, all planes at once."""
    B, A, C, Hf, Wf = x_alpha.shape
    dt, s = x.dtype, float(fov_scale)
    Dc = depth_bins.numel()
    mf = min(Hf, Wf)
    u, t = _source_rays(cams, H, W, s, dt, x.device)
    v = depth_bins.to(dt).view(1, 1, Dc, 1, 1, 1) * u[:, :, None] + t[:, :, None, None, None, :]          # [B,A,Dc,H,W,3]
    w = v[..., 2]
    w = torch.where(w < 0, -torch.ones_like(w), torch.ones_like(w)) * w.abs().clamp(min=1e-8)             # transform_points(eps=1e-8)
    g = torch.cat(((-(mf / Wf) * s) * v[..., 0] / w, (-(mf / Hf) * s) * v[..., 1] / w), 2)                # warp, :176-178
    g = F.interpolate(g.reshape(B * A, 2 * Dc, H, W), size=(Hf, Wf), mode="bicubic", align_corners=False)
    grid = torch.stack((g[:, :Dc], g[:, Dc:]), -1).reshape(B * A, Dc * Hf, Wf, 2)
    # a coordinate that is not finite, or absurdly far out, samples nothing: sent well outside the map before grid_sample converts it
    bad = ~(torch.isfinite(grid) & (grid.abs() < 1e6))
    grid = torch.where(bad, torch.full_like(grid, -3.0), grid)
    smp = F.grid_sample(x_alpha.reshape(B * A, C, Hf, Wf), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    smp = smp.reshape(B, A, C, Dc, Hf, Wf).mean(1)
    return (smp - x[:, :, None]).abs().sum(1) / C


def cost_volume_composite(x, x_alpha, cams, depth_bins, H, W, fov_scale=COST_VOLUME_FOV_SCALE, plane_chunk=8):
    """ops.cost_volume in plain torch (any device, differentiable in x and x_alpha), `plane_chunk` planes at a time: the largest
    intermediates are the [B,A,plane_chunk,H,W,3] source-view points and the [B,A,C,plane_chunk,Hf,Wf] samples."""
    D = depth_bins.numel()
    return torch.cat([cost_volume_planes(x, x_alpha, cams, depth_bins[k:k + plane_chunk], H, W, fov_scale)
                      for k in range(0, D, plane_chunk)], 1)


def _window_moments(x, y):
    """x, y [N,C,H,W] -> (mu_x, mu_y, sigma_x, sigma_y, sigma_xy) over the 3x3 windows of the reflection-padded images, the second
    moments centred on the window's means (upstream's E[y^2] - mu^2 cancels in flat regions, where sigma is small next to C2)."""
    px = F.pad(x, (1, 1, 1, 1), mode="reflect").unfold(2, 3, 1).unfold(3, 3, 1)                            # [N,C,H,W,3,3] views
    py = F.pad(y, (1, 1, 1, 1), mode="reflect").unfold(2, 3, 1).unfold(3, 3, 1)
    mu_x, mu_y = px.mean((-1, -2)), py.mean((-1, -2))
    dx, dy = px - mu_x[..., None, None], py - mu_y[..., None, None]
    return mu_x, mu_y, (dx * dx).mean((-1, -2)), (dy * dy).mean((-1, -2)), (dx * dy).mean((-1, -2))


def ssim_loss(x, y):
    """upstream's SSIM.forward (ManyDepth.py:828-842) of x, y [N,C,H,W], with centred window moments."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y, s_x, s_y, s_xy = _window_moments(x, y)
    n = (2 * mu_x * mu_y + C1) * (2 * s_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (s_x + s_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def reconstruction_loss_composite(images, alpha_images, mask, cams, depth, zfar, ssim_factor, padding_mode="border",
                                  fov_scale=COST_VOLUME_FOV_SCALE, return_map=False, ssim_loss_fn=None):
    """ops.reconstruction_loss in plain torch (any device, depth's dtype; differentiable in depth and in the cameras): upstream's
    reconstruction_loss_fn (macarons_utils.py:1120-1185) for S depth maps.  images [B,H,W,3], alpha_images [B,A,H,W,3], mask [B,H,W]
    bool or None, cams [B,1+A,12], depth [S,B,H,W] -> loss [S] (return_map: also the selected per-pixel loss [S,B,H,W] and its source
    index).  Also what serves the cases the entry does not take: padding_mode 'reflection', cameras that require a gradient, another
    field of view than upstream's default (through fov_scale), an ssim_loss_fn(x, y) of the caller's (None: `ssim_loss` above)."""
    S, B, H, W = depth.shape
    A = alpha_images.shape[1]
    dt, s, f = depth.dtype, float(fov_scale), float(ssim_factor)
    m = min(H, W)
    u, t = _source_rays(cams, H, W, s, dt, depth.device)
    d = depth if mask is None else torch.where(mask[None], depth, torch.full_like(depth, float(zfar)))
    x = images.to(dt).permute(0, 3, 1, 2)[:, None].expand(B, A, 3, H, W).reshape(B * A, 3, H, W)
    src = alpha_images.to(dt).reshape(B * A, H, W, 3).permute(0, 3, 1, 2)
    losses, maps, idxs = [], [], []
    for k in range(S):
        v = d[k][:, None, :, :, None] * u + t[:, :, None, None, :]                                         # [B,A,H,W,3]
        w = v[..., 2]
        w = torch.where(w < 0, -torch.ones_like(w), torch.ones_like(w)) * w.abs().clamp(min=1e-8)
        g = torch.stack(((-(m / W) * s) * v[..., 0] / w, (-(m / H) * s) * v[..., 1] / w), -1).reshape(B * A, H, W, 2)
        # a PIXEL coordinate that is not finite samples nothing -- decided where the entry decides it, on the coordinate rounded to this
        # dtype, so a finite grid coordinate whose pixel coordinate overflows counts as not finite in both; a distant finite one is brought to where
        # grid_sample converts it safely (border: still the border pixel, zeros: still nothing)
        ok = torch.isfinite((((g.double() + 1) * g.new_tensor([W, H], dtype=torch.float64) - 1) / 2).to(dt)).all(-1)
        g = torch.where(ok[..., None], g, torch.zeros_like(g))
        g = torch.where(g.abs() < 1e6, g, torch.full_like(g, -3.0) if padding_mode == "zeros" else g.detach().clamp(-1e6, 1e6))
        y = F.grid_sample(src, g, mode="bilinear", padding_mode=padding_mode, align_corners=False) * ok[:, None].to(dt)
        loss = (x - y).abs().mean(1)
        if f > 0:
            loss = f * (ssim_loss if ssim_loss_fn is None else ssim_loss_fn)(x, y).mean(1) + (1 - f) * loss
        sel, idx = torch.min(loss.reshape(B, A, H, W), dim=1)
        if mask is not None:
            mk = mask.to(dt)
            losses.append((sel * mk / (mk.sum((1, 2), keepdim=True) + 1e-7)).sum())
        else:
            losses.append(sel.mean())
        maps.append(sel), idxs.append(idx)
    if return_map:
        return torch.stack(losses), torch.stack(maps), torch.stack(idxs)
    return torch.stack(losses)


def edge_aware_gradients(disp, img):
    """disp [N,1,H,W], img [N,C,H,W] -> (|disp[.., x] - disp[.., x+1]| exp(-mean_c |img[.., x] - img[.., x+1]|) [N,1,H,W-1], the same
    downwards [N,1,H-1,W]): the two weighted difference maps both of upstream's regularity functions are made of
    (depth_model_utils.py:533-540, :553-560)."""
    gx = (disp[..., :, :-1] - disp[..., :, 1:]).abs() * torch.exp(-(img[..., :, :-1] - img[..., :, 1:]).abs().mean(1, keepdim=True))
    gy = (disp[..., :-1, :] - disp[..., 1:, :]).abs() * torch.exp(-(img[..., :-1, :] - img[..., 1:, :]).abs().mean(1, keepdim=True))
    return gx, gy


def disparity_scales_composite(disps, images, mask, znear, zfar, return_tab=False):
    """ops.disparity_scales in plain torch (any device, the disparities' dtype; differentiable in the disparities): what upstream's
    apply_depth_model does between the depth network and its losses (macarons_utils.py:959-1031).  disps: a sequence of [B,1,H_s,W_s]
    or [B,H_s,W_s] maps of ANY size (F.interpolate, mode 'nearest', brings each to the images' size: this also serves the ratios and
    sizes the entry refuses); images [B,H,W,3]; mask [B,H,W] bool or None.  Returns (depth [S,B,H,W], reg [S], error_mask [B,H,W] bool),
    with return_tab also (tab [B,H,W], thr [B]).  Like the entry it upsamples the disparity itself where upstream upsamples the depth and
    converts back (the identity), and zeroes the masked-out pixels by selection."""
    B, H, W, _ = images.shape
    dt = disps[0].dtype
    a, b = 1.0 / float(znear) - 1.0 / float(zfar), 1.0 / float(zfar)
    img = images.to(dt).permute(0, 3, 1, 2)
    depths, regs, n0 = [], [], None
    for d in disps:
        d = d.reshape(B, 1, d.shape[-2], d.shape[-1])
        if tuple(d.shape[-2:]) != (H, W):
            d = F.interpolate(d, size=(H, W), mode="nearest")
        depths.append(1.0 / (a * d[:, 0] + b))
        n = d / (d.mean((2, 3), keepdim=True) + 1e-7)
        if mask is not None:
            n = torch.where(mask[:, None], n, torch.zeros_like(n))
        gx, gy = edge_aware_gradients(n, img)
        regs.append(gx.mean() + gy.mean())
        if n0 is None:
            n0 = n.detach()
    with torch.no_grad():                                   # the error mask of scale 0 (:984-993): the table of the reflection-padded copies
        gx, gy = edge_aware_gradients(F.pad(n0, (1, 1, 1, 1), mode="reflect"), F.pad(img, (1, 1, 1, 1), mode="reflect"))
        tab = (gx[:, 0, :H, :W] + gy[:, 0, :H, :W])
        thr = tab.reshape(B, -1).mean(-1) + tab.reshape(B, -1).std(-1)
        error_mask = tab < thr.view(B, 1, 1)
    out = (torch.stack(depths), torch.stack(regs), error_mask)
    return out + (tab, thr) if return_tab else out


def _forward(self, x, R, T, zfar, x_alpha, R_alpha, T_alpha, zfar_alpha, device=None, return_cost_volume=False):
    """CostVolumeBuilder.forward (ManyDepth.py:207-305), same signature: x [B,C,Hf,Wf], R [B,3,3], T [B,3], x_alpha [B,A,C,Hf,Wf],
    R_alpha [B,A,3,3], T_alpha [B,A,3] -> relu(conv_reduce(cat(x, cost volume))) [B,output_channels,Hf,Wf] (and the cost volume
    [B,n_depth,Hf,Wf]).  zfar, zfar_alpha and device are accepted and unused: the far planes drop out, the tensors name the device.
    The sweep writes the volume where the cat would put it; with gradients required for x or x_alpha it goes through CostVolumeFunction."""
    from ..autograd import CostVolumeFunction
    # upstream's forward is also where its plain tensor attributes reach the device (ManyDepth.py:225-228; they are no buffers, .to()
    # leaves them behind): depth_bins, and on an adopted upstream instance the pixel tables x_tab / y_tab its reproject_depth_map reads
    for name in ("depth_bins", "x_tab", "y_tab"):
        t = getattr(self, name, None)
        if torch.is_tensor(t) and t.device != x.device:
            setattr(self, name, t.to(x.device))
    B, C, Hf, Wf = x.shape
    cams = pack_cameras(R, T, R_alpha, T_alpha)
    if torch.is_grad_enabled() and (x.requires_grad or x_alpha.requires_grad):
        buf = CostVolumeFunction.apply(x, x_alpha, cams, self.depth_bins, self.height, self.width, COST_VOLUME_FOV_SCALE, True)
    else:
        with torch.no_grad():
            buf = torch.empty((B, C + self.n_depth, Hf, Wf), dtype=torch.float32, device=x.device)
            buf[:, :C].copy_(x)
            ops.cost_volume(x, x_alpha, cams, self.depth_bins, self.height, self.width, out=buf[:, C:])
    res = F.relu(self.conv_reduce(buf))
    if return_cost_volume:
        return res, buf[:, C:]
    return res


class CostVolumeBuilder(nn.Module):
    """Mirror of upstream's CostVolumeBuilder: the same constructor arguments, attributes and parameter names (`conv_reduce.weight`,
    `conv_reduce.bias`: upstream state dicts load), the forward on HIP.  `reproject_depth_map` and `warp` are not offered here; a caller
    that needs them (upstream's reconstruction loss) keeps its upstream instance and adopts it (adopt_cost_volume_builder)."""

    def __init__(self, height, width, feature_height, feature_width, feature_channels, n_alpha, d_min, d_max, n_depth, output_channels,
                 kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.height, self.width = height, width
        self.feature_height, self.feature_width, self.feature_channels = feature_height, feature_width, feature_channels
        self.n_alpha = n_alpha
        self.d_min, self.d_max, self.n_depth = d_min, d_max, n_depth
        self.depth_bins = torch.linspace(d_min, d_max, n_depth)
        self.conv_reduce = nn.Conv2d(in_channels=feature_channels + n_depth, out_channels=output_channels, kernel_size=kernel_size,
                                     stride=stride, padding=padding)
        self.relu = nn.ReLU()

    forward = _forward


_ADOPT_ATTRIBUTES = ("height", "width", "feature_height", "feature_width", "feature_channels", "n_alpha", "d_min", "d_max", "n_depth",
                     "depth_bins", "conv_reduce")


class _AdoptedForward:
    """The `forward` of an adopted instance: a module-level callable holding the instance, so that the instance still pickles
    (torch.save(model)) and deep-copies -- a bound method of a function that upstream's class does not have would not."""

    def __init__(self, builder):
        self.builder = builder

    def __call__(self, *args, **kwargs):
        return _forward(self.builder, *args, **kwargs)


def adopt_cost_volume_builder(builder):
    """Put an existing upstream CostVolumeBuilder instance on the HIP sweep: its `forward` is rebound (on the instance) to the forward
    above, which reads only height, width, feature_*, n_alpha, d_min, d_max, n_depth, depth_bins and conv_reduce, and like upstream's
    moves depth_bins, x_tab and y_tab to the input's device; `reproject_depth_map` and `warp` stay as they are, upstream's
    reconstruction loss calls them.  Returns the instance; adopting twice changes nothing.  Loading a pickled adopted model needs this
    package importable.

        adopt_cost_volume_builder(macarons.depth.depth_decoder.cost_volume_builder)"""
    missing = [a for a in _ADOPT_ATTRIBUTES if not hasattr(builder, a)]
    if missing:
        raise TypeError(f"adopt_cost_volume_builder: not a CostVolumeBuilder, it lacks {missing}")
    if not isinstance(vars(builder).get("forward"), _AdoptedForward):
        object.__setattr__(builder, "forward", _AdoptedForward(builder))     # a plain instance attribute, whatever the class's __setattr__ does
    return builder


# ---- the disparity heads ---------------------------------------------------------------------------------------------------------------------
def disparity_head_composite(x, weight, bias):
    """ops.disparity_head in plain torch (any device and dtype, differentiable): upstream's DisparityLayer.forward as the three ops
    torch runs it as -- the reflection-padded copy, the convolution, the sigmoid.  x [B,C,Hs,Ws], weight [1,C,3,3], bias [1] ->
    [B,1,Hs,Ws]."""
    return torch.sigmoid(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), weight, bias))


def _head_forward(self, x):
    """DisparityLayer.forward (ManyDepth.py:383-384), same signature: x [B,C,Hs,Ws] -> sigmoid(conv(x)) [B,1,Hs,Ws].  Without a gradient
    to record, contiguous float32 HIP tensors outside autocast go to the fused entry (profiles/disparity_head_times.json: faster than
    upstream's op sequence at all four of upstream's shapes, the intervals apart at B 1 and B 4); anything else (CPU, another dtype,
    autocast, a strided input) is served by the composite.  With a gradient required the route follows
    autograd.disparity_head_backward_mode(): 'hip' (MCR_DISPARITY_HEAD_BWD=hip) goes through DisparityHeadFunction, the default
    'composite' runs the composite under autograd -- upstream's own sequence: the same file shows the step through the Function faster
    with the intervals apart at nine rows of ten, not at all of them, which is what the project's rule asks of a default."""
    w, b = self.conv.weight, self.conv.bias
    fused = (x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and w.device == x.device and x.dim() == 4
             and x.is_contiguous() and w.is_contiguous() and not torch.is_autocast_enabled()
             and x.shape[1] <= ops.DISPARITY_HEAD_MAX_CHANNELS and min(x.shape[2:]) >= 2 and x.numel() < 2 ** 31)
    if fused and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
        from ..autograd import DisparityHeadFunction, disparity_head_backward_mode
        if disparity_head_backward_mode() == "hip":
            return DisparityHeadFunction.apply(x, w, b)
        fused = False
    return ops.disparity_head(x, w, b) if fused else disparity_head_composite(x, w, b)


class DisparityLayer(nn.Module):
    """Mirror of upstream's DisparityLayer: the same constructor argument, attributes and parameter names (`conv.weight` [1,C,3,3],
    `conv.bias` [1]: upstream state dicts load).  The forward is the HIP entry wherever no gradient is recorded; with a gradient
    required it is the torch composite under autograd by default and the HIP function with MCR_DISPARITY_HEAD_BWD=hip (_head_forward)."""

    def __init__(self, input_channels):
        super().__init__()
        self.channels = input_channels
        self.conv = nn.Conv2d(in_channels=input_channels, out_channels=1, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
        self.sigmoid = nn.Sigmoid()

    forward = _head_forward


class _AdoptedHeadForward:
    """The `forward` of an adopted DisparityLayer: a module-level callable holding the instance (see _AdoptedForward)."""

    def __init__(self, layer):
        self.layer = layer

    def __call__(self, x):
        return _head_forward(self.layer, x)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def adopt_disparity_layer(layer):
    """Put an existing upstream DisparityLayer instance on the HIP head: its `forward` is rebound (on the instance) to the forward above,
    which reads only `conv.weight` and `conv.bias`.  TypeError unless `conv` is what the entry computes: a 3 x 3, stride 1, padding 1,
    `reflect`, one-output-channel, ungrouped, undilated convolution with a bias.  Returns the instance; adopting twice changes nothing.
    Loading a pickled adopted model needs this package importable."""
    conv = getattr(layer, "conv", None)
    facts = None if conv is None else [
        ("kernel_size", (3, 3)), ("stride", (1, 1)), ("padding", (1, 1)), ("dilation", (1, 1)), ("padding_mode", "reflect"),
        ("out_channels", 1), ("groups", 1)]
    if facts is None or not all(hasattr(conv, k) for k, _ in facts) or getattr(conv, "bias", None) is None:
        raise TypeError("adopt_disparity_layer: not a DisparityLayer, it has no `conv` with a bias and a convolution's attributes")
    wrong = [f"{k} = {getattr(conv, k)!r}" for k, v in facts if (_pair(getattr(conv, k)) if isinstance(v, tuple) else getattr(conv, k)) != v]
    if wrong:
        raise TypeError("adopt_disparity_layer: the head is a 3 x 3, stride 1, padding 1, reflect, one-output-channel convolution; this "
                        f"one has {', '.join(wrong)}")
    if not isinstance(vars(layer).get("forward"), _AdoptedHeadForward):
        object.__setattr__(layer, "forward", _AdoptedHeadForward(layer))
    return layer


# ---- the expansion layers ----------------------------------------------------------------------------------------------------------------------
EXPANSION_LAYER_DEFAULT = "composite"          # what profiles/expansion_layer_times.json decides (see _expansion_forward)


def expansion_layer_mode():
    """'composite' or 'hip': the route of an expansion layer's forward when no gradient is recorded.  MCR_EXPANSION_LAYER=hip or
    =composite chooses; otherwise EXPANSION_LAYER_DEFAULT, which is 'hip' only if profiles/expansion_layer_times.json shows the fused
    entry faster than the composite with the intervals apart at all five of upstream's shapes, at B 1 and at B 4."""
    import os
    mode = os.environ.get("MCR_EXPANSION_LAYER", "").strip().lower()
    return mode if mode in ("hip", "composite") else EXPANSION_LAYER_DEFAULT


def expansion_layer_composite(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size):
    """ops.expansion_layer in plain torch (any device and dtype, differentiable): upstream's ExpansionLayer.forward as the seven ops torch
    runs it as -- the transposed convolution, ELU, the nearest resize, the concatenation (with an x_add), the reflection-padded copy, the
    convolution, ELU.  x [B,Cin,h,w], x_add [B,Cadd,H,W] or None, up_weight [Cin,Cmid,3,3], i_weight [Cout,Cmid+Cadd,3,3] -> [B,Cout,H,W]."""
    u = F.elu(F.conv_transpose2d(x, up_weight, up_bias, stride=1, padding=1))
    r = F.interpolate(u, size=tuple(int(v) for v in output_size), mode="nearest")
    if x_add is not None:
        r = torch.cat((r, x_add), dim=-3)
    return F.elu(F.conv2d(F.pad(r, (1, 1, 1, 1), mode="reflect"), i_weight, i_bias))


def _is_hip_tensor(t):
    return t.is_cuda


def _autocast_on(x):
    """Autocast is enabled for the device type of x."""
    try:
        return torch.is_autocast_enabled(x.device.type)
    except TypeError:                                             # a torch whose is_autocast_enabled takes no device type
        return torch.is_autocast_enabled() if x.is_cuda else torch.is_autocast_cpu_enabled()


def expansion_layer_route(x, x_add, params, output_size, additional_channels):
    """'hip', 'function' or 'composite' for one forward.  The fused entry serves contiguous float32 HIP tensors outside autocast, within
    the entry's limits: 'hip' (ops.expansion_layer) when no gradient is recorded and the mode (expansion_layer_mode) is 'hip';
    'function' (autograd.ExpansionLayerFunction: the fused forward and the HIP backward) when a gradient is to be recorded and
    autograd.expansion_layer_backward_mode() is 'hip' (MCR_EXPANSION_LAYER_BWD=hip; MCR_EXPANSION_LAYER, the knob of the forward without
    a gradient, has no say there).  params: (upconv.weight, upconv.bias, iconv.weight, iconv.bias).  An x_add that the layer ignores
    (additional_channels None) is not an operand."""
    if additional_channels is None:
        x_add = None
    elif x_add is None:
        return "composite"                                       # upstream's own forward fails there; the composite fails the same way
    ts = [x, *params] + ([x_add] if x_add is not None else [])
    if not all(isinstance(t, torch.Tensor) for t in ts):
        return "composite"
    recorded = torch.is_grad_enabled() and any(t.requires_grad for t in ts)
    if recorded:
        from ..autograd import expansion_layer_backward_mode
        if expansion_layer_backward_mode() != "hip":
            return "composite"                                   # upstream's sequence under autograd: the HIP backward is opt-in
    elif expansion_layer_mode() != "hip":
        return "composite"
    if _autocast_on(x):
        return "composite"
    if not all(_is_hip_tensor(t) and t.device == x.device and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        return "composite"
    cap = ops.EXPANSION_LAYER_MAX_CHANNELS
    wu, _, wi, _ = params
    if x.dim() != 4 or wu.dim() != 4 or wi.dim() != 4 or (x_add is not None and x_add.dim() != 4):
        return "composite"
    H, W = (int(v) for v in output_size)
    B, Cin, Cmid, Cout, Ctot = x.shape[0], x.shape[1], wu.shape[1], wi.shape[0], wi.shape[1]
    if B < 1 or min(x.shape[2:]) < 1 or min(H, W) < 2 or not (1 <= Cin <= cap and 1 <= Cmid <= cap and 1 <= Cout <= cap and Ctot <= cap):
        return "composite"
    if max(x.numel(), B * Cmid * x.shape[2] * x.shape[3], B * Ctot * H * W, B * Cout * H * W) >= 2 ** 31:
        return "composite"
    if recorded and B * Ctot * (H + 2) * (W + 2) >= 2 ** 31:
        return "composite"                                       # the backward's G carries the ring
    return "function" if recorded else "hip"


def _expansion_forward(self, x, x_add=None):
    """ExpansionLayer.forward (ManyDepth.py:351-363), same signature: x [B,Cin,h,w], x_add [B,Cadd,H,W] -> [B,Cout,H,W]; like upstream's,
    x_add is concatenated only when both it and additional_channels are set.  The route is expansion_layer_route: the fused entry
    (ops.expansion_layer) without a gradient to record under the mode 'hip'; with a gradient required, ExpansionLayerFunction under
    MCR_EXPANSION_LAYER_BWD=hip and the composite under autograd otherwise (the default); the composite for everything the entry does
    not take."""
    if x_add is not None and self.additional_channels is None:
        x_add = None
    params = (self.upconv.weight, self.upconv.bias, self.iconv.weight, self.iconv.bias)
    route = expansion_layer_route(x, x_add, params, self.output_size, self.additional_channels)
    if route == "hip":
        return ops.expansion_layer(x, x_add, *params, self.output_size)
    if route == "function":
        from ..autograd import ExpansionLayerFunction
        return ExpansionLayerFunction.apply(x, x_add, *params, self.output_size)
    return expansion_layer_composite(x, x_add, *params, self.output_size)


class ExpansionLayer(nn.Module):
    """Mirror of upstream's ExpansionLayer: the same constructor arguments, attributes and parameter names (`upconv.weight`
    [Cin,Cmid,3,3], `upconv.bias`, `iconv.weight` [Cout,Cmid+Cadd,3,3], `iconv.bias`: upstream state dicts load).  The forward is
    _expansion_forward."""

    def __init__(self, input_channels, inner_channels, output_channels, output_size, additional_channels=None, kernel_size=3, stride=1,
                 padding=1):
        super().__init__()
        self.upconv = nn.ConvTranspose2d(in_channels=input_channels, out_channels=inner_channels, kernel_size=kernel_size, stride=stride,
                                         padding=padding)
        self.upelu = nn.ELU()
        total_inner_channels = inner_channels + (additional_channels if additional_channels is not None else 0)
        self.iconv = nn.Conv2d(in_channels=total_inner_channels, out_channels=output_channels, kernel_size=kernel_size, stride=stride,
                               padding=padding, padding_mode="reflect")
        self.ielu = nn.ELU()
        self.input_channels, self.output_channels, self.output_size = input_channels, output_channels, output_size
        self.inner_channels, self.additional_channels = inner_channels, additional_channels
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding

    def upsample(self, x):
        return F.interpolate(input=x, size=self.output_size, mode="nearest")

    forward = _expansion_forward


class _AdoptedExpansionForward:
    """The `forward` of an adopted ExpansionLayer: a module-level callable holding the instance (see _AdoptedForward)."""

    def __init__(self, layer):
        self.layer = layer

    def __call__(self, x, x_add=None):
        return _expansion_forward(self.layer, x, x_add)


def adopt_expansion_layer(layer):
    """Put an existing upstream ExpansionLayer instance on the forward above: its `forward` is rebound (on the instance); it reads
    `upconv`, `iconv`, `output_size` and `additional_channels`.  TypeError unless the layer is what the entry computes: `upconv` a 3 x 3,
    stride 1, padding 1, output-padding 0, undilated, ungrouped transposed convolution with a bias; `iconv` a 3 x 3, stride 1, padding 1,
    `reflect`, undilated, ungrouped convolution with a bias; both ELUs with alpha 1; `output_size` a pair of ints.  Returns the instance;
    adopting twice changes nothing.  Loading a pickled adopted model needs this package importable."""
    who = "adopt_expansion_layer"
    common = [("kernel_size", (3, 3)), ("stride", (1, 1)), ("padding", (1, 1)), ("dilation", (1, 1)), ("groups", 1)]
    facts = {"upconv": common + [("output_padding", (0, 0))], "iconv": common + [("padding_mode", "reflect")]}
    wrong = []
    for name, wanted in facts.items():
        conv = getattr(layer, name, None)
        if conv is None or not all(hasattr(conv, k) for k, _ in wanted) or getattr(conv, "bias", None) is None \
                or not torch.is_tensor(getattr(conv, "weight", None)):
            raise TypeError(f"{who}: not an ExpansionLayer, it has no `{name}` with a weight, a bias and a convolution's attributes")
        wrong += [f"{name}.{k} = {getattr(conv, k)!r}" for k, v in wanted
                  if (_pair(getattr(conv, k)) if isinstance(v, tuple) else getattr(conv, k)) != v]
    if layer.upconv.weight.dim() != 4 or layer.iconv.weight.dim() != 4:
        raise TypeError(f"{who}: the convolutions are not two-dimensional")
    for name in ("upelu", "ielu"):
        elu = getattr(layer, name, None)
        if elu is None or not hasattr(elu, "alpha"):
            raise TypeError(f"{who}: not an ExpansionLayer, it has no `{name}` with an alpha")
        if float(elu.alpha) != 1.0:
            wrong.append(f"{name}.alpha = {elu.alpha!r}")
    size = getattr(layer, "output_size", None)
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in size)):
        wrong.append(f"output_size = {size!r}")
    if not hasattr(layer, "additional_channels"):
        raise TypeError(f"{who}: not an ExpansionLayer, it has no `additional_channels`")
    if wrong:
        raise TypeError(f"{who}: the layer is a 3 x 3, stride 1, padding 1 transposed convolution, ELU, a nearest resize to a pair of ints "
                        f"and a 3 x 3, stride 1, padding 1, reflect convolution, ELU; this one has {', '.join(wrong)}")
    if not isinstance(vars(layer).get("forward"), _AdoptedExpansionForward):
        object.__setattr__(layer, "forward", _AdoptedExpansionForward(layer))
    return layer


_EXPANSION_NAMES = ("expansion1", "expansion2", "expansion3", "expansion4", "expansion5")


def adopt_depth_decoder(decoder):
    """adopt_cost_volume_builder(decoder.cost_volume_builder), adopt_disparity_layer on decoder.disp1 .. disp4 and adopt_expansion_layer on
    decoder.expansion1 .. expansion5 (upstream's DepthDecoder, ManyDepth.py:387-529).  A decoder with none of the five expansion layers
    is adopted without them; one with some of them only is refused (TypeError).  Returns the decoder.

        adopt_depth_decoder(macarons.depth.depth_decoder)"""
    names = ("cost_volume_builder", "disp1", "disp2", "disp3", "disp4")
    missing = [a for a in names if not hasattr(decoder, a)]
    if missing:
        raise TypeError(f"adopt_depth_decoder: not a DepthDecoder, it lacks {missing}")
    present = [a for a in _EXPANSION_NAMES if hasattr(decoder, a)]
    if present and len(present) != len(_EXPANSION_NAMES):
        raise TypeError(f"adopt_depth_decoder: the decoder has {present} but lacks {[a for a in _EXPANSION_NAMES if a not in present]}")
    adopt_cost_volume_builder(decoder.cost_volume_builder)
    for name in names[1:]:
        adopt_disparity_layer(getattr(decoder, name))
    for name in present:
        adopt_expansion_layer(getattr(decoder, name))
    return decoder


# ---- the front of the ResNet encoder: the feature extractor ---------------------------------------------------------------------------------
FEATURE_EXTRACTOR_DEFAULT = "hip"              # what profiles/feature_extractor_times.json decides (see feature_extractor_mode)


def feature_extractor_mode():
    """'composite' or 'hip': the route of the feature extractor in eval mode when no gradient is recorded.  MCR_FEATURE_EXTRACTOR=hip or
    =composite chooses; otherwise FEATURE_EXTRACTOR_DEFAULT, which is 'hip' only if profiles/feature_extractor_times.json shows the whole
    extractor through the adopted route below upstream's piecewise sequence with the intervals apart, at B 1 and at B 4."""
    import os
    mode = os.environ.get("MCR_FEATURE_EXTRACTOR", "").strip().lower()
    return mode if mode in ("hip", "composite") else FEATURE_EXTRACTOR_DEFAULT


def _batch_norm_eval(z, bn, eps):
    weight, bias, mean, var = bn
    return F.batch_norm(z, mean, var, weight, bias, False, 0.0, eps)


def resnet_stem_composite(x, weight, bias, bn, eps):
    """ops.resnet_stem in plain torch (any device and dtype): the four ops upstream runs -- the 7 x 7 / 2 convolution, the BatchNorm on
    its running statistics (bn = (weight, bias, running_mean, running_var)), ReLU, the 3 x 3 / 2 max-pool.  x [N,Cin,H,W] -> (pooled,
    conv1), conv1 the map after ReLU."""
    conv1 = F.relu(_batch_norm_eval(F.conv2d(x, weight, bias, stride=2, padding=3), bn, eps))
    return F.max_pool2d(conv1, kernel_size=3, stride=2, padding=1), conv1


def basic_block_composite(x, w1, bn1, eps1, w2, bn2, eps2, stride=1, downsample=None):
    """ops.basic_block in plain torch (any device and dtype): torchvision's BasicBlock.forward with both BatchNorms on their running
    statistics -- and with the stride of the first convolution and the `downsample` of the identity, which the entry does not serve."""
    t = F.relu(_batch_norm_eval(F.conv2d(x, w1, None, stride=stride, padding=1), bn1, eps1))
    y = _batch_norm_eval(F.conv2d(t, w2, None, stride=1, padding=1), bn2, eps2)
    return F.relu(y + (x if downsample is None else downsample(x)))


def feature_extractor_composite(x, weight, bias, bn, eps, blocks):
    """ops.feature_extractor in plain torch on one image operand: the stem, then every (w1, bn1, eps1, w2, bn2, eps2) of `blocks`.
    -> (features, conv1)."""
    y, conv1 = resnet_stem_composite(x, weight, bias, bn, eps)
    for blk in blocks:
        y = basic_block_composite(y, *blk)
    return y, conv1


def _bn_operands(bn):
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var), float(bn.eps)


def _block_operands(block):
    bn1, eps1 = _bn_operands(block.bn1)
    bn2, eps2 = _bn_operands(block.bn2)
    return (block.conv1.weight, bn1, eps1, block.conv2.weight, bn2, eps2)


def _flat(operands):
    for t in operands:
        if isinstance(t, (tuple, list)):
            yield from _flat(t)
        elif torch.is_tensor(t):
            yield t


def _conv_facts(name, conv, wanted):
    """The attributes of `conv` that differ from `wanted`, as 'name.attribute = value' strings (a missing one reads as None)."""
    wrong = []
    for k, v in wanted:
        got = getattr(conv, k, None)
        if (_pair(got) if isinstance(v, tuple) and got is not None else got) != v:
            wrong.append(f"{name}.{k} = {got!r}")
    return wrong


def _bn_facts(name, bn):
    wrong = []
    for k in ("weight", "bias", "running_mean", "running_var"):
        if not torch.is_tensor(getattr(bn, k, None)):
            wrong.append(f"{name}.{k} = {getattr(bn, k, None)!r}")
    if not isinstance(getattr(bn, "eps", None), float):
        wrong.append(f"{name}.eps = {getattr(bn, 'eps', None)!r}")
    return wrong


_BLOCK_CONV = [("kernel_size", (3, 3)), ("stride", (1, 1)), ("padding", (1, 1)), ("dilation", (1, 1)), ("groups", 1), ("padding_mode", "zeros"),
               ("bias", None)]


def _block_facts(name, block):
    """What keeps a basic block from the entry: its convolutions are 3 x 3 / 1 / 1, zeros, without bias, its BatchNorms affine with running
    statistics, its stride 1 and its downsample None."""
    parts = [p for p in ("conv1", "bn1", "conv2", "bn2") if not hasattr(block, p)]
    if parts:
        return [f"{name} lacks {parts}"]
    wrong = _conv_facts(f"{name}.conv1", block.conv1, _BLOCK_CONV) + _conv_facts(f"{name}.conv2", block.conv2, _BLOCK_CONV)
    wrong += _bn_facts(f"{name}.bn1", block.bn1) + _bn_facts(f"{name}.bn2", block.bn2)
    if getattr(block, "downsample", None) is not None:
        wrong.append(f"{name}.downsample = {type(block.downsample).__name__}")
    if getattr(block, "stride", 1) not in (1, (1, 1)):
        wrong.append(f"{name}.stride = {block.stride!r}")
    for a, b in (("conv1", "conv2"),):
        wa, wb = getattr(block.conv1, "weight", None), getattr(block.conv2, "weight", None)
        if not (torch.is_tensor(wa) and torch.is_tensor(wb) and wa.dim() == 4 and wa.shape == wb.shape and wa.shape[0] == wa.shape[1]):
            wrong.append(f"{name}: {a}.weight and {b}.weight are not two [C,C,3,3]")
    return wrong


def _extractor_blocks(fe):
    layer = fe.layer
    try:
        return list(layer)
    except TypeError:
        return None


def _extractor_facts(fe):
    """What keeps a feature extractor (conv1, bn1, relu, maxpool, layer) from the entry, as strings; empty: the entry computes it."""
    wrong = _conv_facts("conv1", fe.conv1, [("kernel_size", (7, 7)), ("stride", (2, 2)), ("padding", (3, 3)), ("dilation", (1, 1)),
                                            ("groups", 1), ("padding_mode", "zeros")])
    if not (torch.is_tensor(getattr(fe.conv1, "weight", None)) and fe.conv1.weight.dim() == 4):
        wrong.append("conv1.weight is not [Cout,Cin,7,7]")
    wrong += _bn_facts("bn1", fe.bn1)
    wrong += _conv_facts("maxpool", fe.maxpool, [("kernel_size", (3, 3)), ("stride", (2, 2)), ("padding", (1, 1)), ("dilation", (1, 1)),
                                                 ("ceil_mode", False), ("return_indices", False)])
    if not isinstance(fe.relu, nn.ReLU):
        wrong.append(f"relu = {type(fe.relu).__name__}")
    blocks = _extractor_blocks(fe)
    if blocks is None or len(blocks) > ops.FEATURE_EXTRACTOR_MAX_BLOCKS:
        wrong.append(f"layer is not a sequence of at most {ops.FEATURE_EXTRACTOR_MAX_BLOCKS} blocks")
    else:
        for k, block in enumerate(blocks):
            wrong += _block_facts(f"layer[{k}]", block)
    return wrong


def _extractor_operands(fe):
    """(weight, bias, bn, eps, blocks): the arguments of ops.feature_extractor after the images."""
    bn, eps = _bn_operands(fe.bn1)
    return fe.conv1.weight, fe.conv1.bias, bn, eps, [_block_operands(b) for b in _extractor_blocks(fe)]


def _hip_operands_ok(images, operands):
    """Contiguous float32 tensors on one HIP device, outside autocast, none to be differentiated."""
    ts = [t for t in images if t is not None] + list(_flat(operands))
    x = ts[0]
    if not all(isinstance(t, torch.Tensor) for t in ts) or _autocast_on(x):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return False
    return all(_is_hip_tensor(t) and t.device == x.device and t.dtype == torch.float32 and t.is_contiguous() for t in ts)


def feature_extractor_route(fe, x, x_more=None):
    """'hip' or 'composite' for one pass of the extractor over x [N0,Cin,H,W] and, in the same call, x_more [N1,Cin,H,W].  'hip'
    (ops.feature_extractor) only when every BatchNorm involved has training == False, no gradient is to be recorded, the tensors are
    contiguous float32 on one HIP device outside autocast and within the entry's limits, the extractor is what the entry computes
    (_extractor_facts) and the mode (feature_extractor_mode) is 'hip'.  Anything else is upstream's own sequence of modules."""
    if feature_extractor_mode() != "hip":
        return "composite"
    if not all(hasattr(fe, a) for a in ("conv1", "bn1", "relu", "maxpool", "layer")) or _extractor_facts(fe):
        return "composite"
    blocks = _extractor_blocks(fe)
    if fe.bn1.training or any(b.bn1.training or b.bn2.training for b in blocks):
        return "composite"
    images = [t for t in (x, x_more) if t is not None]
    if not images or not all(isinstance(t, torch.Tensor) and t.dim() == 4 and t.shape[1:] == images[0].shape[1:] for t in images):
        return "composite"
    if not _hip_operands_ok(images, _extractor_operands(fe)):
        return "composite"
    w = fe.conv1.weight
    N, (Cin, H, W), Cout = sum(int(t.shape[0]) for t in images), (int(v) for v in images[0].shape[1:]), int(w.shape[0])
    if N < 1 or H < 1 or W < 1 or w.shape[1] != Cin or not (1 <= Cin <= ops.RESNET_STEM_MAX_CIN and 1 <= Cout <= ops.RESNET_STEM_MAX_COUT):
        return "composite"
    if any(b.conv1.weight.shape[0] != Cout for b in blocks):
        return "composite"
    Hc, Wc, _, _ = ops.resnet_stem_sizes(H, W)
    if max(N * Cin * H * W, N * Cout * Hc * Wc) >= 2 ** 31:
        return "composite"
    return "hip"


def _extractor_pieces(fe, x):
    """Upstream's own sequence on one image operand (ManyDepth.py:486-491) -> (features, conv1)."""
    conv1 = fe.relu(fe.bn1(fe.conv1(x)))
    return fe.layer(fe.maxpool(conv1)), conv1


def extractor_front(fe, x, sources):
    """(features of x, features of sources, conv1 of x) as the decoder's forward needs them: where feature_extractor_route says 'hip', ONE
    ops.feature_extractor call for both operands; otherwise the extractor's modules piece by piece on x and then on the sources, as
    upstream calls them (ManyDepth.py:486-500)."""
    if feature_extractor_route(fe, x, sources) == "hip":
        features, conv1 = ops.feature_extractor(x, sources, *_extractor_operands(fe))
        return features[:x.shape[0]], features[x.shape[0]:], conv1
    layer1, conv1 = _extractor_pieces(fe, x)
    return layer1, _extractor_pieces(fe, sources)[0], conv1


def _extractor_forward(self, x):
    """FeatureExtractor.forward (ManyDepth.py:43-50), same signature: x [N,Cin,H,W] -> layer(maxpool(relu(bn1(conv1(x))))).  The route is
    feature_extractor_route: one fused entry in eval mode without a gradient under the mode 'hip', the modules themselves otherwise."""
    if feature_extractor_route(self, x) == "hip":
        return ops.feature_extractor(x, None, *_extractor_operands(self), want_conv1=False)[0]
    return _extractor_pieces(self, x)[0]


def _block_forward(self, x):
    """torchvision's BasicBlock.forward, the module sequence and nothing else: a block on its own is never routed to HIP (inside a
    FeatureExtractor on the HIP route the extractor's entry takes the blocks' operands and this forward does not run)."""
    out = self.relu(self.bn1(self.conv1(x)))
    out = self.bn2(self.conv2(out))
    return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class BasicBlock(nn.Module):
    """Mirror of torchvision's BasicBlock (torchvision is not needed): the same constructor arguments, attributes and state-dict names
    (`conv1.weight`, `bn1.*`, `conv2.weight`, `bn2.*`, `downsample.*`), so that a resnet18 state dict loads.  Its forward is torch's modules (_block_forward);
    the fused entry serves it as part of a FeatureExtractor, where stride and downsample are refused."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    forward = _block_forward


class FeatureExtractor(nn.Module):
    """Mirror of upstream's FeatureExtractor: the same constructor (anything with conv1, bn1, relu, maxpool and layer1) and attribute
    names (`conv1`, `bn1`, `relu`, `maxpool`, `layer`).  The forward is _extractor_forward."""

    def __init__(self, resnet_model):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = resnet_model.conv1, resnet_model.bn1, resnet_model.relu, resnet_model.maxpool
        self.layer = resnet_model.layer1

    forward = _extractor_forward


class _AdoptedExtractorForward:
    """The `forward` of an adopted FeatureExtractor: a module-level callable holding the instance (see _AdoptedForward)."""

    def __init__(self, extractor):
        self.extractor = extractor

    def __call__(self, x):
        return _extractor_forward(self.extractor, x)


def adopt_feature_extractor(fe):
    """Put an existing upstream FeatureExtractor instance on the forward above: its `forward` is rebound (on the instance); it reads
    `conv1`, `bn1`, `relu`, `maxpool` and `layer`.  TypeError, naming every wrong fact, unless the extractor is what the entry computes: a
    7 x 7, stride 2, padding 3, zeros, undilated, ungrouped convolution; a BatchNorm with affine parameters and running statistics; ReLU;
    a 3 x 3, stride 2, padding 1, undilated max-pool without ceil_mode; at most four blocks of two 3 x 3, stride 1, padding 1 convolutions
    without bias and two such BatchNorms, without stride or downsample.  Returns the instance; adopting twice changes nothing.  Loading a
    pickled adopted model needs this package importable."""
    who = "adopt_feature_extractor"
    missing = [a for a in ("conv1", "bn1", "relu", "maxpool", "layer") if not hasattr(fe, a)]
    if missing:
        raise TypeError(f"{who}: not a FeatureExtractor, it lacks {missing}")
    wrong = _extractor_facts(fe)
    if wrong:
        raise TypeError(f"{who}: the extractor is a 7 x 7, stride 2, padding 3 convolution, a BatchNorm with affine parameters and running "
                        "statistics, ReLU, a 3 x 3, stride 2, padding 1 max-pool and blocks of 3 x 3, stride 1, padding 1 convolutions without "
                        f"bias or downsample; this one has {', '.join(wrong)}")
    if not isinstance(vars(fe).get("forward"), _AdoptedExtractorForward):
        object.__setattr__(fe, "forward", _AdoptedExtractorForward(fe))
    return fe


def _depth_forward(self, x, R, T, zfar, x_alpha, R_alpha, T_alpha, zfar_alpha, device):
    """DepthDecoder.forward (ManyDepth.py:474-531), same signature and the same attribute names: x [B,C,H,W], x_alpha [B,A,C,H,W] ->
    (disp1, disp2, disp3, disp4).  The one difference is the front: where feature_extractor_route says 'hip', the target and the A source
    images of every batch element go through ops.feature_extractor in ONE call (in eval mode BatchNorm is per image, so no value changes),
    the map after the first ReLU kept for the target alone; otherwise the extractor's modules are called piece by piece on x and then on
    the sources, as upstream calls them."""
    fe = self.feature_extractor
    B, A = x.shape[0], x_alpha.shape[1]
    sources = x_alpha.reshape(-1, self.channels, self.height, self.width)
    layer1, layer1_alpha, conv1 = extractor_front(fe, x, sources)
    layer1_alpha = layer1_alpha.view(B, A, 64, self.height // 4, self.width // 4)
    reduced = self.cost_volume_builder(layer1, R, T, zfar, layer1_alpha, R_alpha, T_alpha, zfar_alpha, device=device)
    layer2 = self.resnet_layer_2(reduced)
    layer3 = self.resnet_layer_3(layer2)
    layer4 = self.resnet_layer_4(layer3)
    iconv5 = self.expansion5(x=layer4, x_add=layer3)
    iconv4 = self.expansion4(x=iconv5, x_add=layer2)
    iconv3 = self.expansion3(x=iconv4, x_add=layer1)
    iconv2 = self.expansion2(x=iconv3, x_add=conv1)
    iconv1 = self.expansion1(x=iconv2, x_add=x if self.use_input_image_in_skip_connection else None)
    return self.disp1(iconv1), self.disp2(iconv2), self.disp3(iconv3), self.disp4(iconv4)


class _AdoptedDepthForward:
    """The `forward` of a decoder after adopt_depth_front: a module-level callable holding the instance (see _AdoptedForward)."""

    def __init__(self, decoder):
        self.decoder = decoder

    def __call__(self, *args, **kwargs):
        return _depth_forward(self.decoder, *args, **kwargs)


_DEPTH_FRONT_ATTRIBUTES = ("feature_extractor", "cost_volume_builder", "resnet_layer_2", "resnet_layer_3", "resnet_layer_4", "disp1", "disp2",
                           "disp3", "disp4", "height", "width", "channels", "use_input_image_in_skip_connection") + _EXPANSION_NAMES


def adopt_depth_front(decoder):
    """Put the front of an existing upstream DepthDecoder on one extractor call: upstream's forward calls the extractor's parts one by one
    (ManyDepth.py:486-500), so adopting the extractor alone does not reach it; this adopts decoder.feature_extractor
    (adopt_feature_extractor, with its refusals) and rebinds the decoder's `forward` (on the instance) to _depth_forward, which is
    upstream's forward from the cost volume on.  adopt_depth_decoder is independent of it; calling both is the usual combination:

        adopt_depth_front(adopt_depth_decoder(macarons.depth.depth_decoder))

    TypeError if the decoder lacks an attribute that forward reads.  Returns the decoder; adopting twice changes nothing."""
    missing = [a for a in _DEPTH_FRONT_ATTRIBUTES if not hasattr(decoder, a)]
    if missing:
        raise TypeError(f"adopt_depth_front: not a DepthDecoder, it lacks {missing}")
    adopt_feature_extractor(decoder.feature_extractor)
    if not isinstance(vars(decoder).get("forward"), _AdoptedDepthForward):
        object.__setattr__(decoder, "forward", _AdoptedDepthForward(decoder))
    return decoder
