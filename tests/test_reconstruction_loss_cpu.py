"""The depth module's photometric reconstruction loss without a GPU: the product's torch composite against the reference's own function
(tests/golden/reconstruction_loss.npz) and against the independent fp64 model (tests/_reconstruction_model.py), the C ABI's declarations
and workspace arithmetic, the signature of the function that get_reconstruction_loss_fn returns, and the patch.

Bounds.  TOL = 1e-4 of the largest magnitude is the project's contract.  The golden carries upstream's fp32 cancellation (its window
moments are E[y^2] - mu^2; the composite's are centred), so against the golden the bound is TOL plus the golden's own distance to the
model, which the generator measured and stored.  The composite in fp64 and the model state the same mathematics with no shared code:
1e-9.  For d_depth the model is forced to the index map under test (either source is a valid subgradient at a near-tie).

Distances measured (max |difference| / max |reference|), composite fp32 vs golden, worst variant of a case:
  loss a 4.5e-07 b 4.6e-07 c 1.5e-06 d 1.2e-06   map a 4.8e-05 b 3.1e-05 c 4.9e-05 d 1.5e-05   d_depth a 3.8e-05 b 5.4e-05 c 1.0e-05 d 8.4e-05
  (the golden's own distance to the model is about the same: the composite sits beside the model, the golden apart from both)
  through the function: fov 45 degrees vs model loss 7.4e-09 d_depth 7.7e-06; cameras with a gradient loss 2.2e-08 d T_alpha 5.4e-07
  composite fp64 vs model: at most 2.1e-14.

The last section holds the cases at the kernels' edges (tests/_depth_loss_cases.py), for which there is no golden: what each reaches in
the kernels' own numbers, the conditions on their inputs from the model alone, and the composite in fp64 against the model (1e-9; measured
loss 2.8e-16, map 2.7e-14, d_depth 1.8e-13 at most).
"""
import ctypes
import inspect
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _reconstruction_model as model                                  # noqa: E402
from _reconstruction_model import VARIANTS, load_case, load_result, rel  # noqa: E402

from macarons_amd import _lib                                          # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

TOL = 1e-4
ALL = [(t, p, m) for t in "abcd" for p, m in VARIANTS[t]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {t: load_case(t) for t in "abcd"}


def _cams(c):
    return ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"], c["T_alpha"])


def _model_args(c, masked):
    return (c["images"], c["alpha_images"], c["mask"] if masked else None, c["R"], c["T"], c["R_alpha"], c["T_alpha"])


@pytest.mark.parametrize("tag,padding,masked", ALL)
def test_composite_fp32_matches_golden(cases, tag, padding, masked):
    c, want = cases[tag], load_result(tag, padding, masked)
    d = c["depth"].clone().requires_grad_(True)
    loss, lmap, idx = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"] if masked else None, _cams(c), d,
                                                              c["zfar"], c["ssim_factor"], padding, return_map=True)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (c["depth"].shape[0],) and lmap.shape == d.shape
    grad = torch.autograd.grad(loss.sum(), d)[0]
    g_loss, g_map, g_grad = (float(v) for v in want["distance"])
    e_loss, e_map, e_grad = rel(loss, want["loss"]), rel(lmap, want["map"]), rel(grad, want["d_depth"])
    n_idx = int((idx != want["index"].long()).sum())
    print(f"case {tag} {padding} mask={masked}: composite fp32 vs golden: loss {e_loss:.2e} map {e_map:.2e} d_depth {e_grad:.2e} "
          f"index differences {n_idx} (golden vs model: {g_loss:.1e} {g_map:.1e} {g_grad:.1e})")
    differ = idx != want["index"].long()
    if n_idx:                                                           # the index: equal, or different only at near-ties of the model
        margin = model.reconstruction(*_model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding)["margin"]
        assert float(margin[differ].max()) < 1e-3 * float(want["map"].max()) and float(differ.double().mean()) <= 0.05
    assert e_loss < TOL + g_loss and e_map < TOL + g_map
    if n_idx == 0:
        assert e_grad < TOL + g_grad
    else:                                                               # a near-tie the two fp32 evaluations broke differently
        m = model.reconstruction(*_model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding)
        differ = idx != want["index"].long()
        assert float(m["margin"][differ].max()) < 1e-3 * float(m["map"].max()) and float(differ.double().mean()) <= 0.05
        ref = model.gradient(*_model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, force_index=idx)
        assert rel(grad, ref) < TOL


@pytest.mark.parametrize("tag,padding,masked", ALL)
def test_composite_fp64_matches_model(cases, tag, padding, masked):
    c = cases[tag]
    d = c["depth"].double().requires_grad_(True)
    d_loss = torch.linspace(0.5, 1.5, d.shape[0], dtype=torch.float64)
    loss, lmap, idx = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"] if masked else None, _cams(c).double(),
                                                              d, c["zfar"], c["ssim_factor"], padding, return_map=True)
    grad = torch.autograd.grad((loss * d_loss).sum(), d)[0]
    with torch.no_grad():
        m = model.reconstruction(*_model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding)
    ref = model.gradient(*_model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, d_loss=d_loss, force_index=idx)
    e = (rel(loss, m["loss"]), rel(lmap, m["map"]), rel(grad, ref))
    print(f"case {tag} {padding} mask={masked}: composite fp64 vs model: loss {e[0]:.2e} map {e[1]:.2e} d_depth {e[2]:.2e}")
    # the cameras reach the composite in fp32 (pack_cameras), as they reach the entry; the model reads the same fp32 values
    assert torch.equal(idx, m["index"]) and max(e) < 1e-9


def test_masked_pixels_warp_at_zfar_and_carry_no_gradient(cases):
    c = cases["a"]
    d = c["depth"].double().requires_grad_(True)
    loss = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"], _cams(c).double(), d, c["zfar"],
                                                   c["ssim_factor"], "border")
    grad = torch.autograd.grad(loss.sum(), d)[0]
    hole = ~c["mask"][None].expand_as(grad)
    assert bool(hole.any()) and bool((grad[hole] == 0).all()) and bool((grad[~hole] != 0).any())


def test_reflection_padding_and_custom_ssim_run_through_the_composite(cases):
    c = cases["c"]
    args = (c["images"], c["alpha_images"], c["mask"], _cams(c), c["depth"], c["zfar"], c["ssim_factor"])
    refl = ManyDepth.reconstruction_loss_composite(*args, "reflection")
    bord = ManyDepth.reconstruction_loss_composite(*args, "border")
    assert bool(torch.isfinite(refl).all()) and not torch.equal(refl, bord)
    d = c["depth"].double().requires_grad_(True)
    l6, m6, i6 = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"], _cams(c).double(), d, c["zfar"],
                                                         c["ssim_factor"], "reflection", return_map=True)
    with torch.no_grad():
        m = model.reconstruction(*_model_args(c, True), c["depth"], c["zfar"], c["ssim_factor"], "reflection")
    ref = model.gradient(*_model_args(c, True), c["depth"], c["zfar"], c["ssim_factor"], "reflection", force_index=i6)
    assert torch.equal(i6, m["index"]) and max(rel(l6, m["loss"]), rel(m6, m["map"]), rel(torch.autograd.grad(l6.sum(), d)[0], ref)) < 1e-9
    half = ManyDepth.reconstruction_loss_composite(*args, "border", ssim_loss_fn=lambda x, y: 0.5 * ManyDepth.ssim_loss(x, y))
    l1 = ManyDepth.reconstruction_loss_composite(*args[:-1], 0.0, "border")
    assert float(half) < float(bord) and float(l1) != float(bord)


def _stand_ins(c, fov=None, grad=False):
    cameras = SimpleNamespace(R=c["R"], T=c["T"])
    alpha_cameras = SimpleNamespace(R=c["R_alpha"].reshape(-1, 3, 3), T=c["T_alpha"].reshape(-1, 3).clone().requires_grad_(grad))
    if fov is not None:
        cameras.fov, alpha_cameras.fov = torch.full((c["R"].shape[0],), fov), torch.full((alpha_cameras.R.shape[0],), fov)
    return cameras, alpha_cameras


def test_other_field_of_view_takes_the_composite(cases):
    """Cameras whose fov is not 60 degrees: the function serves them through the composite with their scale, on any device, and the
    value and depth gradient are the model's at that scale; the same fov on both objects is one field of view, two are refused."""
    import math
    from macarons_amd.utility import macarons_utils as mu
    c = cases["b"]
    B, A, H, W, _ = c["alpha_images"].shape
    params = SimpleNamespace(use_depth_mask=True, zfar=c["zfar"], ssim_factor=c["ssim_factor"])
    cameras, alpha_cameras = _stand_ins(c, fov=45.0)
    scale = 1.0 / math.tan(math.radians(45.0) / 2)
    assert mu._fov_scale_of(cameras, alpha_cameras) == (scale, False)
    assert mu._fov_scale_of(*_stand_ins(c)) == mu._fov_scale_of(*_stand_ins(c, fov=60.0)) == (model.FOV_SCALE, True)
    leaf = c["depth"][0].reshape(B, H, W, 1).clone().requires_grad_(True)
    got = mu.get_reconstruction_loss_fn(params)(params, c["images"], c["alpha_images"], c["mask"][..., None], cameras, alpha_cameras, leaf,
                                                None, None)
    got.backward()
    with torch.no_grad():
        idx = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"], _cams(c), c["depth"], c["zfar"],
                                                      c["ssim_factor"], "border", scale, return_map=True)[2]
        m = model.reconstruction(*_model_args(c, True), c["depth"], c["zfar"], c["ssim_factor"], "border", fov_scale=scale)
        m60 = model.reconstruction(*_model_args(c, True), c["depth"], c["zfar"], c["ssim_factor"], "border")
    ref = model.gradient(*_model_args(c, True), c["depth"], c["zfar"], c["ssim_factor"], "border", force_index=idx, fov_scale=scale)
    e_loss, e_grad = rel(got, m["loss"][0]), rel(leaf.grad.reshape(1, B, H, W), ref)
    print(f"fov 45 through the function (composite, fp32) vs model: loss {e_loss:.2e} d_depth {e_grad:.2e}")
    assert e_loss < TOL and e_grad < TOL and rel(m60["loss"], m["loss"]) > 100 * TOL
    alpha_cameras.fov = torch.full((B * A,), 60.0)
    with pytest.raises(ValueError, match="one field of view"):
        mu._fov_scale_of(cameras, alpha_cameras)


def test_cameras_that_require_a_gradient_take_the_composite(cases):
    """Source translations that require a gradient: the function serves them through the composite and d loss / d T_alpha is the model's."""
    from macarons_amd.utility import macarons_utils as mu
    c = cases["b"]
    B, A, H, W, _ = c["alpha_images"].shape
    params = SimpleNamespace(use_depth_mask=True, zfar=c["zfar"], ssim_factor=c["ssim_factor"])
    cameras, alpha_cameras = _stand_ins(c, grad=True)
    got = mu.get_reconstruction_loss_fn(params)(params, c["images"], c["alpha_images"], c["mask"][..., None], cameras, alpha_cameras,
                                                c["depth"][0].reshape(B, H, W, 1), None, None)
    got.backward()
    with torch.no_grad():
        idx = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"], _cams(c), c["depth"], c["zfar"],
                                                      c["ssim_factor"], "border", return_map=True)[2]
    Ta6 = c["T_alpha"].double().requires_grad_(True)
    m = model.reconstruction(c["images"], c["alpha_images"], c["mask"], c["R"], c["T"], c["R_alpha"], Ta6, c["depth"], c["zfar"],
                             c["ssim_factor"], "border", force_index=idx)
    ref = torch.autograd.grad(m["loss"].sum(), Ta6)[0]
    e_loss, e_grad = rel(got, m["loss"][0]), rel(alpha_cameras.T.grad.reshape(B, A, 3), ref)
    print(f"cameras with a gradient through the function (composite, fp32) vs model: loss {e_loss:.2e} d T_alpha {e_grad:.2e}")
    assert e_loss < TOL and e_grad < TOL and float(ref.abs().max()) > 0


def test_pixel_coordinate_that_overflows_samples_nothing(cases):
    """A finite grid coordinate whose pixel coordinate overflows fp32 is not finite where the entry decides it: the composite samples
    nothing there either, in both padding modes (case c's first source alone, 3e38 units off: the grid coordinate is finite, 3e37 or more,
    and 20 times that is not; no SSIM part, so the loss is the mean of |I|)."""
    c = cases["c"]
    cams = ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"][:, :1], torch.tensor([[[3e38, 0.0, 0.0]]]))
    for padding in ("border", "zeros"):
        loss = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"][:, :1], None, cams, c["depth"], c["zfar"], 0.0, padding)
        assert torch.allclose(loss[0], c["images"].abs().mean(), rtol=1e-6, atol=0)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("mcr_reconstruction_loss_workspace_bytes", "mcr_reconstruction_loss", "mcr_reconstruction_loss_backward_workspace_bytes",
           "mcr_reconstruction_loss_backward")


def test_symbols_declared_and_exported():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n


def test_workspace_arithmetic():
    L = _lib.lib()
    i64 = ctypes.c_int64
    fwd, bwd = L.mcr_reconstruction_loss_workspace_bytes, L.mcr_reconstruction_loss_backward_workspace_bytes
    assert fwd.restype is ctypes.c_size_t and bwd.restype is ctypes.c_size_t

    def up(v):
        return (v + 255) // 256 * 256

    for S, B, A, H, W in ((1, 1, 1, 2, 2), (2, 2, 2, 20, 28), (1, 2, 2, 19, 37), (4, 4, 2, 256, 456), (3, 5, 8, 33, 16)):
        n = S * B * ((H + 15) // 16) * ((W + 15) // 16)                  # one partial sum and one mask count per 16 x 16 tile
        assert fwd(i64(S), i64(B), i64(A), i64(H), i64(W)) == 2 * up(4 * n) + up(8 * S * B), (S, B, A, H, W)
        assert bwd(i64(S), i64(B), i64(A), i64(H), i64(W)) == up(4 * 64 * B)                  # 64 partial mask counts an image
    for S, B, A, H, W in ((0, 1, 1, 4, 4), (1, 0, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 9, 4, 4), (1, 1, 2, 1, 4), (1, 1, 2, 4, 1),
                          (1, 1, 2, -4, 4), (70000, 1, 2, 4, 4), (1, 70000, 2, 4, 4), (1, 1, 2, 2 ** 20, 2 ** 20),
                          (60000, 60000, 8, 2 ** 15, 2 ** 15)):
        assert fwd(i64(S), i64(B), i64(A), i64(H), i64(W)) == 0, (S, B, A, H, W)
        assert bwd(i64(S), i64(B), i64(A), i64(H), i64(W)) == 0, (S, B, A, H, W)


# ---- upstream's interface ------------------------------------------------------------------------------------------------------------
def test_returned_function_has_upstream_parameters():
    from macarons_amd.utility import macarons_utils as mu
    fn = mu.get_reconstruction_loss_fn(SimpleNamespace())
    ps = inspect.signature(fn).parameters
    assert list(ps) == model.parameter_names()
    assert ps["channel_is_at_the_end"].default is True and ps["padding_mode"].default == "border"
    assert list(inspect.signature(mu.get_reconstruction_loss_fn).parameters) == ["params"]
    assert list(inspect.signature(mu.reconstruction_losses).parameters)[:7] == ["params", "images", "alpha_images", "mask", "cameras",
                                                                               "alpha_cameras", "depths"]


def test_fn_takes_the_composite_for_what_the_entry_does_not(cases):
    """Reflection padding is served by the composite, on any device: the function called on CPU tensors returns the composite's value in
    both channel orders (the entry would refuse a CPU tensor)."""
    from macarons_amd.utility import macarons_utils as mu
    c = cases["b"]
    B, A, H, W, _ = c["alpha_images"].shape
    params = SimpleNamespace(use_depth_mask=True, zfar=c["zfar"], ssim_factor=c["ssim_factor"])
    cameras = SimpleNamespace(R=c["R"], T=c["T"])
    alpha_cameras = SimpleNamespace(R=c["R_alpha"].reshape(-1, 3, 3), T=c["T_alpha"].reshape(-1, 3))
    fn = mu.get_reconstruction_loss_fn(params)
    want = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"], _cams(c), c["depth"], c["zfar"],
                                                   c["ssim_factor"], "reflection")[0]
    depth = c["depth"][0].reshape(B, H, W, 1)
    last = fn(params, c["images"], c["alpha_images"], c["mask"][..., None], cameras, alpha_cameras, depth, None, None, True, "reflection")
    first = fn(params, c["images"].permute(0, 3, 1, 2), c["alpha_images"].permute(0, 1, 4, 2, 3), c["mask"][..., None], cameras,
               alpha_cameras, depth, None, None, channel_is_at_the_end=False, padding_mode="reflection")
    assert torch.equal(last, want) and torch.equal(first, want)
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # border is the entry's: no fall-back to torch on the CPU
        fn(params, c["images"], c["alpha_images"], c["mask"][..., None], cameras, alpha_cameras, depth, None, None)


def test_patch_reference_reports_the_helper():
    import test_patch_reference as TP
    if not os.path.isdir(os.path.join(TP.REFERENCE, "macarons")):
        pytest.skip("needs the MACARONS reference source tree, which is not part of this repository")
    TP._run("""
    import macarons.utility.macarons_utils as ref
    ref_fn = ref.get_reconstruction_loss_fn
    import macarons_amd
    from macarons_amd.utility import macarons_utils as mu
    rep = macarons_amd.patch_reference(helpers="all")
    assert ref.get_reconstruction_loss_fn is mu.get_reconstruction_loss_fn
    assert ("macarons.utility.macarons_utils", "get_reconstruction_loss_fn") in rep["helpers"]
    from macarons_amd.patch import unpatch_reference
    unpatch_reference()
    assert ref.get_reconstruction_loss_fn is ref_fn
    print("__OK__")
    """)


def test_patch_lists_the_helper():
    from macarons_amd import patch
    assert "get_reconstruction_loss_fn" in patch._HELPERS_ALL["utility.macarons_utils"][1]
    assert "get_reconstruction_loss_fn" not in patch._HELPERS["utility.macarons_utils"][1]


# ---- the cases at the kernels' edges (tests/_depth_loss_cases.py): what they reach, their conditions, and the reference itself -------------
import _depth_loss_cases as edge                                       # noqa: E402

EDGE_ALL = [(t, p, m) for t in edge.RECONSTRUCTION_TAGS for p, m in edge.RECONSTRUCTION_VARIANTS[t]]


@pytest.fixture(scope="module")
def edge_cases():
    return {t: edge.reconstruction_case(t) for t in edge.RECONSTRUCTION_TAGS}


def test_edge_cases_reach_what_they_are_for(edge_cases):
    """The sizes in the kernels' own numbers, so that a later change of RL_T or of the chunk counts cannot silently empty a case:
    tiles66 has more tiles than rl_finish_kernel has lanes and more pixels than one pass of rl_mask_count_kernel's 64 x 256 threads;
    pairs6 has more (scale, image) pairs than rl_finish_kernel has waves; pairs6_dark has one image fully masked and one not; spill1's last
    tile row and column hold one image row / column; rows3 has H = 3 and a two-column spill."""
    S, B, H, W = edge_cases["tiles66"]["depth"].shape
    assert edge.cdiv(H, 16) * edge.cdiv(W, 16) > 64 and edge.n_tiles(H, W) > edge.FINISH_LANES
    assert H * W > 64 * 256 and H * W > edge.COUNT_CHUNKS * edge.COUNT_THREADS
    assert edge.cdiv(H * W, edge.COUNT_CHUNKS) > edge.COUNT_THREADS                         # every chunk takes the second step
    mask = edge_cases["tiles66"]["mask"]
    assert bool((~mask).any()) and bool(mask.reshape(-1)[-edge.cdiv(H * W, edge.COUNT_CHUNKS):].all())   # and a dropped term is a set pixel
    for tag in ("pairs6", "pairs6_dark"):
        S, B, H, W = edge_cases[tag]["depth"].shape
        assert S * B > 4 and S * B > edge.FINISH_WAVES and B > 1 and edge.n_tiles(H, W) > 1
    assert not torch.equal(edge_cases["pairs6"]["depth"][2], edge_cases["pairs6"]["depth"][0])
    dark = edge_cases["pairs6_dark"]["mask"]
    assert not bool(dark[1].any()) and bool(dark[0].any()) and not bool(dark[0].all())
    S, B, H, W = edge_cases["spill1"]["depth"].shape
    assert H % edge.TILE == 1 and W % edge.TILE == 1 and H > edge.TILE and W > edge.TILE and B == 2
    S, B, H, W = edge_cases["rows3"]["depth"].shape
    assert H == 3 and W % edge.TILE == 2 and W > edge.TILE


@pytest.mark.parametrize("tag,padding,masked", EDGE_ALL)
def test_edge_conditions_and_composite_fp64_matches_model(edge_cases, tag, padding, masked):
    """The conditions on the inputs, from the model alone -- at most 5 % of the pixels are near-ties (two best sources within 1e-3 of
    the map's maximum), both sources are selected, tiles66 has at most 2 % kink pixels by test_upstream_width's rule, and the gradient is
    not zero where a case looks for it -- and the check that the reference is right at the new shapes, for which there is no golden: the
    composite in fp64 and the model state the same mathematics with no shared code, 1e-9 as for cases a-d."""
    c = edge_cases[tag]
    S, B, H, W = c["depth"].shape
    d_loss = edge.D_LOSS[S].double()
    with torch.no_grad():
        m = model.reconstruction(*edge.model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding)
    ties = edge.near_tie_share(m)
    shares = [float((m["index"] == a).double().mean()) for a in range(c["alpha_images"].shape[1])]
    msg = f"edge case {tag} {padding} mask={masked}: near-ties {100 * ties:.2f} % of the pixels; selected {['%.0f %%' % (100 * s) for s in shares]}"
    if tag == "tiles66":
        kink = float(edge.kinks(c, m).double().mean())
        msg += f"; kink pixels {100 * kink:.2f} %"
        assert kink <= edge.MAX_KINKS
    assert ties <= edge.MAX_NEAR_TIES and min(shares) > 0.1
    d = c["depth"].double().requires_grad_(True)
    loss, lmap, idx = ManyDepth.reconstruction_loss_composite(c["images"], c["alpha_images"], c["mask"] if masked else None, _cams(c).double(),
                                                              d, c["zfar"], c["ssim_factor"], padding, return_map=True)
    grad = torch.autograd.grad((loss * d_loss).sum(), d)[0]
    ref = model.gradient(*edge.model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, d_loss=d_loss, force_index=idx)
    e = (rel(loss, m["loss"]), rel(lmap, m["map"]), rel(grad, ref))
    print(msg + f"; composite fp64 vs model: loss {e[0]:.2e} map {e[1]:.2e} d_depth {e[2]:.2e}")
    assert torch.equal(idx, m["index"]) and max(e) < 1e-9
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(m["loss"]).all())
    if tag == "pairs6_dark":                                            # the fully masked image: no loss, exactly no gradient
        assert bool((ref[:, 1] == 0).all()) and bool((grad[:, 1] == 0).all()) and bool((ref[:, 0] != 0).any())
    if tag == "spill1":                                                 # the spill row and column, and their reflected partners
        assert all(bool((ref[0, b, r] != 0).any()) and bool((ref[0, b, :, q] != 0).any()) for b in range(B) for r in (H - 2, H - 1)
                   for q in (W - 2, W - 1))
    if tag == "rows3":
        assert bool((ref[0, 0, 1] != 0).any()) and bool((ref[0, 0, :, W - 2:] != 0).any())
