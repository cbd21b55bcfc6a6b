"""The disparity-scales step of the depth module without a GPU: the product's torch composite (networks.ManyDepth.disparity_scales_composite)
against the independent fp64 model (tests/_disparity_model.py) and against the reference's own functions
(tests/golden/disparity_scales.npz), the four mirrors with upstream's names, depth_scale_losses on its composite route, the C ABI's
declarations and workspace arithmetic, the argument refusals and the patch.

Bounds.  TOL = 1e-4 of the largest magnitude is the project's contract (`rel` of tests/_reconstruction_model.py: max |a - b| / max |b|).
Against the golden the bound is TOL plus the golden's own distance to the model, which the generator measured and stored (at most 3.7e-6).
The error mask must equal the model's at every pixel that is not undecided (|tab - thr| < 1e-4 thr in the model).

Distances measured, composite fp32 vs model, worst case: depth 9.3e-08 reg 1.3e-07 tab 2.8e-06 thr 1.6e-07 d_disp 2.0e-07;
composite fp64 vs golden (that is, the golden's own fp32 rounding): depth 9.3e-08 reg 1.3e-07 tab 3.7e-06 thr 2.5e-07 d_disp 2.0e-07.

The last section holds the cases at the kernels' edges (tests/_depth_loss_cases.py), for which there is no golden: what each reaches in
the kernels' own numbers, the golden generator's conditions on their inputs from the model alone, and the composite in fp64 against the
model (1e-9; measured 1.8e-15 at most).
"""
import ctypes
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _disparity_model as model                                       # noqa: E402
from _reconstruction_model import rel                                  # noqa: E402
import _reconstruction_model as rmodel                                 # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402
from macarons_amd.utility import macarons_utils as mu                  # noqa: E402

TOL = 1e-4
PARAMS = SimpleNamespace(znear=model.ZNEAR, zfar=model.ZFAR)


def t(x):
    return torch.as_tensor(np.asarray(x))


@pytest.fixture(scope="module")
def cases():
    return {tag: model.load_case(tag) for tag in model.GOLDEN_TAGS}


@pytest.fixture(scope="module")
def modelled(cases):
    """The fp64 model of every variant, computed once and never changed."""
    return {(tag, m): model.forward(cases[tag]["disps"], cases[tag]["images"], cases[tag]["mask"] if m else None) for tag, m in model.VARIANTS}


def _composite(c, masked, dtype, c_reg, g_depth):
    leaves = [t(d).to(dtype).requires_grad_(True) for d in c["disps"]]
    depth, reg, em, tab, thr = ManyDepth.disparity_scales_composite(leaves, t(c["images"]), t(c["mask"]) if masked else None, model.ZNEAR,
                                                                    model.ZFAR, return_tab=True)
    grads = torch.autograd.grad((reg * t(c_reg).to(dtype)).sum() + (depth * t(g_depth).to(dtype)).sum(), leaves)
    return depth, reg, em, tab, thr, grads


@pytest.mark.parametrize("tag,masked", model.VARIANTS)
def test_composite_fp32_matches_model(cases, modelled, tag, masked):
    c, m, want = cases[tag], modelled[tag, masked], model.load_result(tag, masked)
    depth, reg, em, tab, thr, grads = _composite(c, masked, torch.float32, want["c"], want["g"])
    assert depth.dtype == torch.float32 and tuple(depth.shape) == m["depth"].shape and em.dtype == torch.bool
    ref = model.gradient(c["disps"], c["images"], c["mask"] if masked else None, want["g"], want["c"])
    e = dict(depth=rel(depth, t(m["depth"])), reg=rel(reg, t(m["reg"])), tab=rel(tab, t(m["tab"])), thr=rel(thr, t(m["thr"])),
             d_disp=max(rel(g, t(r)) for g, r in zip(grads, ref)))
    undecided = model.conditions(c["disps"], c["images"], c["mask"] if masked else None)[3]
    print(f"case {tag} mask={masked}: composite fp32 vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL
    assert all(tuple(g.shape) == d.shape for g, d in zip(grads, c["disps"]))
    assert bool(((em.numpy() == m["error_mask"]) | undecided).all())


@pytest.mark.parametrize("tag,masked", model.VARIANTS)
def test_composite_fp64_matches_golden(cases, tag, masked):
    c, want = cases[tag], model.load_result(tag, masked)
    depth, reg, em, tab, thr, grads = _composite(c, masked, torch.float64, want["c"], want["g"])
    assert depth.dtype == torch.float64
    e = dict(depth=rel(depth, t(want["depth"])), reg=rel(reg, t(want["reg"])), tab=rel(tab, t(want["tab"])), thr=rel(thr, t(want["thr"])),
             d_disp=max(rel(g, t(r)) for g, r in zip(grads, want["d_disp"])))
    print(f"case {tag} mask={masked}: composite fp64 vs golden: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f" (golden vs model: {want['distance']})")
    for k, v in e.items():
        assert v < TOL + want["distance"][k], k
    undecided = model.conditions(c["disps"], c["images"], c["mask"] if masked else None)[3]
    assert bool(((em.numpy() == want["error_mask"]) | undecided).all())


def test_fully_masked_image_gives_zeros(cases):
    """Case e: image 1 is fully masked -- its table is 0, its error mask all false, and the regularity half of its gradient exactly 0."""
    c = cases["e"]
    leaves = [t(d).double().requires_grad_(True) for d in c["disps"]]
    depth, reg, em, tab, thr = ManyDepth.disparity_scales_composite(leaves, t(c["images"]), t(c["mask"]), model.ZNEAR, model.ZFAR, return_tab=True)
    grad = torch.autograd.grad(reg.sum(), leaves)[0]
    assert bool((tab[1] == 0).all()) and float(thr[1]) == 0 and not bool(em[1].any()) and bool(em[0].any())
    assert bool((grad[1] == 0).all()) and bool((grad[0] != 0).any())
    alone = ManyDepth.disparity_scales_composite([leaves[0][:1]], t(c["images"])[:1], t(c["mask"])[:1], model.ZNEAR, model.ZFAR)[1]
    assert rel(reg * 2, alone) < 1e-12                                  # image 1 adds nothing to the sum, only to the count


def test_gradcheck_of_the_fp64_composite():
    """Case a shrunk to 8 x 8 (ratios 1, 2, 4, 8: the coarsest map is one pixel), through depth and reg."""
    rng = np.random.default_rng(21)
    B, H, W = 2, 8, 8
    images = t(model.smooth_images(rng, B, H, W))
    disps = [model.smooth_disparity(rng, B, H // r, W // r) for r in (1, 2, 4, 8)]
    mask = torch.ones(B, H, W, dtype=torch.bool)
    mask[:, 2:5, 3:6] = False
    assert model.conditions(disps, images.numpy(), mask.numpy())[0] >= 1e-4
    leaves = [t(d).double().requires_grad_(True) for d in disps]
    assert torch.autograd.gradcheck(lambda *d: ManyDepth.disparity_scales_composite(d, images, mask, model.ZNEAR, model.ZFAR)[:2], leaves,
                                    eps=1e-7, atol=1e-7, rtol=1e-5)


def test_other_sizes_go_through_interpolate(cases):
    """A map that is 3 times smaller, and one of an unrelated size, are served by the composite as F.interpolate(mode='nearest') reads them."""
    rng = np.random.default_rng(22)
    images = t(model.smooth_images(rng, 1, 12, 18))
    d3, odd = t(model.smooth_disparity(rng, 1, 4, 6)), t(model.smooth_disparity(rng, 1, 5, 7))
    depth, reg, em = ManyDepth.disparity_scales_composite([d3[:, None], odd], images, None, model.ZNEAR, model.ZFAR)
    up3 = d3.repeat_interleave(3, 1).repeat_interleave(3, 2)
    want = model.forward([up3.numpy()], images.numpy(), None)
    assert tuple(depth.shape) == (2, 1, 12, 18) and rel(depth[0], t(want["depth"][0])) < TOL and rel(reg[0], t(want["reg"][0])) < TOL
    up = F.interpolate(odd[:, None], size=(12, 18), mode="nearest")[:, 0]
    assert rel(reg[1], t(model.forward([up.numpy()], images.numpy(), None)["reg"][0])) < TOL


# ---- the mirrors with upstream's names ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked", model.VARIANTS)
def test_upstream_named_mirrors_match_golden(cases, modelled, tag, masked):
    c, m, want = cases[tag], modelled[tag, masked], model.load_result(tag, masked)
    disp0, img = t(c["disps"][0])[:, None], t(c["images"]).permute(0, 3, 1, 2)
    depth0 = mu.compute_depth_from_disparity(PARAMS, disp0)
    assert rel(depth0[:, 0], t(want["depth"][0])) < TOL + want["distance"]["depth"]
    assert rel(mu.compute_disparity_from_depth(PARAMS, t(want["depth"][0])), disp0[:, 0]) < TOL + want["distance"]["depth"]
    fn = mu.get_regularity_loss_fn(PARAMS)
    for s in range(len(c["disps"])):
        n = t(m["n"][s]).float()[:, None]
        assert rel(fn(disp=n, img=img), t(want["reg"][s])) < TOL + want["distance"]["reg"]
    n0 = t(m["n"][0]).float()[:, None]
    tab = mu.regularity_tab(disp=F.pad(n0, (1, 1, 1, 1), mode="reflect"), img=F.pad(img, (1, 1, 1, 1), mode="reflect"))
    assert tuple(tab.shape) == (n0.shape[0], 1) + tuple(n0.shape[-2:])
    assert rel(tab[:, 0], t(want["tab"])) < TOL + want["distance"]["tab"]


def test_mirrors_have_upstream_parameter_lists():
    assert list(inspect.signature(mu.compute_depth_from_disparity).parameters) == ["params", "disp"]
    assert list(inspect.signature(mu.compute_disparity_from_depth).parameters) == ["params", "depth"]
    assert list(inspect.signature(mu.regularity_tab).parameters) == ["disp", "img"]
    assert list(inspect.signature(mu.get_regularity_loss_fn).parameters) == ["params"]
    assert list(inspect.signature(mu.get_regularity_loss_fn(PARAMS)).parameters) == ["disp", "img"]
    assert list(inspect.signature(mu.depth_scale_losses).parameters) == ["params", "disps", "images", "alpha_images", "mask", "cameras",
                                                                        "alpha_cameras", "padding_mode", "ssim_loss_fn", "compute_loss"]


# ---- depth_scale_losses on the route that needs no GPU ------------------------------------------------------------------------------------
def test_depth_scale_losses_composite_route():
    """Maps of sizes the entry does not take, with reflection padding: both calls go through the composites, on the CPU, and the result
    is the chain written out by hand; without the regularity loss its half is 0. and carries no gradient."""
    rc = rmodel.load_case("a")                                          # images, sources, cameras and mask of the reconstruction golden
    B, A, H, W, _ = rc["alpha_images"].shape
    rng = np.random.default_rng(23)
    disps = [t(model.smooth_disparity(rng, B, 10, 13))[:, None], t(model.smooth_disparity(rng, B, 7, 9))[:, None]]
    params = SimpleNamespace(znear=0.5, zfar=rc["zfar"], ssim_factor=rc["ssim_factor"], use_depth_mask=True, regularity_loss=True,
                             regularity_factor=0.3)
    cameras = SimpleNamespace(R=rc["R"], T=rc["T"])
    alpha_cameras = SimpleNamespace(R=rc["R_alpha"].reshape(-1, 3, 3), T=rc["T_alpha"].reshape(-1, 3))
    leaves = [d.clone().requires_grad_(True) for d in disps]
    dl, rl, depth, mask, em = mu.depth_scale_losses(params, leaves, rc["images"], rc["alpha_images"], rc["mask"][..., None], cameras,
                                                    alpha_cameras, "reflection")
    (dl + rl).backward()
    mine = [d.clone().requires_grad_(True) for d in disps]
    d2, r2, e2 = ManyDepth.disparity_scales_composite(mine, rc["images"], rc["mask"], 0.5, rc["zfar"])
    cams = ManyDepth.pack_cameras(rc["R"], rc["T"], rc["R_alpha"], rc["T_alpha"])
    l2 = ManyDepth.reconstruction_loss_composite(rc["images"], rc["alpha_images"], rc["mask"], cams, d2, rc["zfar"], rc["ssim_factor"], "reflection")
    (l2.sum() + 0.3 * (r2[0] + 0.5 * r2[1])).backward()
    assert torch.allclose(dl, l2.sum()) and torch.allclose(rl, 0.3 * (r2[0] + 0.5 * r2[1]))
    assert tuple(depth.shape) == (B, H, W, 1) and not depth.requires_grad and torch.equal(depth[..., 0], d2[0].detach())
    assert tuple(mask.shape) == (B, H, W, 1) and mask.dtype == torch.bool and tuple(em.shape) == (B, H, W, 1) and torch.equal(em[..., 0], e2)
    for a, b in zip(leaves, mine):
        assert rel(a.grad, b.grad) < 1e-5
    params.regularity_factor = 0.0
    dl0, rl0, *_ = mu.depth_scale_losses(params, leaves, rc["images"], rc["alpha_images"], rc["mask"][..., None], cameras, alpha_cameras,
                                         "reflection")
    assert rl0 == 0. and isinstance(rl0, float) and torch.allclose(dl0, dl)
    out = mu.depth_scale_losses(params, leaves, rc["images"], rc["alpha_images"], rc["mask"][..., None], cameras, alpha_cameras, "reflection",
                                compute_loss=False)
    assert out[0] == 0. and out[1] == 0. and not out[2].requires_grad and torch.equal(out[2], depth) and torch.equal(out[4], em)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_raise_value_error():
    images = torch.zeros(2, 12, 24, 3)
    full = torch.zeros(2, 1, 12, 24)
    for bad in ([full, torch.zeros(2, 1, 4, 8)],                        # ratio 3
                [full, torch.zeros(2, 1, 6, 8)],                        # 2 down, 3 across
                [full, torch.zeros(2, 1, 6, 11)],                       # a mismatched size
                [full, torch.zeros(3, 1, 6, 12)],                       # another batch
                [full] * 9,                                             # S = 9
                []):
        with pytest.raises(ValueError):
            ops.disparity_scales(bad, images, None, 0.5, 750.0)
        with pytest.raises(ValueError):
            ops.disparity_scales_backward(bad, images, None, 0.5, 750.0, None, torch.zeros(max(len(bad), 1)))
    with pytest.raises(ValueError):
        ops.disparity_scales([full], images, torch.ones(2, 12, 23, dtype=torch.bool), 0.5, 750.0)
    with pytest.raises(ValueError):
        ops.disparity_scales_backward([full], images, None, 0.5, 750.0, None, None)
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # well-formed CPU tensors: no fall-back to torch
        ops.disparity_scales([full], images, None, 0.5, 750.0)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("mcr_disparity_scales_workspace_bytes", "mcr_disparity_scales", "mcr_disparity_scales_backward_workspace_bytes",
           "mcr_disparity_scales_backward")


def test_symbols_declared_and_exported():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n


def test_workspace_arithmetic():
    L = _lib.lib()
    i64 = ctypes.c_int64
    fwd, bwd = L.mcr_disparity_scales_workspace_bytes, L.mcr_disparity_scales_backward_workspace_bytes
    assert fwd.restype is ctypes.c_size_t and bwd.restype is ctypes.c_size_t

    def up(v):
        return (v + 255) // 256 * 256

    for S, B, H, W in ((1, 1, 2, 3), (4, 2, 16, 24), (2, 2, 19, 37), (4, 4, 256, 456), (8, 3, 33, 16)):
        tiles = ((H + 15) // 16) * ((W + 15) // 16)
        means = up(8 * 32 * S * B)                                      # 32 double partial sums per scale and image
        assert fwd(i64(S), i64(B), i64(H), i64(W)) == (means + up(4 * 2 * S * B * tiles) + up(8 * 2 * B * tiles) + up(8 * (2 * S * B + 2 * B))
                                                       + up(4 * B * H * W) + up(4 * B)), (S, B, H, W)
        assert bwd(i64(S), i64(B), i64(H), i64(W)) == means + up(8 * S * B * tiles), (S, B, H, W)
    for S, B, H, W in ((0, 1, 4, 4), (9, 1, 4, 4), (1, 0, 4, 4), (1, 1, 1, 4), (1, 1, 4, 1), (1, 1, -4, 4), (1, 70000, 4, 4),
                       (1, 1, 2 ** 20, 2 ** 20), (8, 60000, 2 ** 15, 2 ** 15)):
        assert fwd(i64(S), i64(B), i64(H), i64(W)) == 0, (S, B, H, W)
        assert bwd(i64(S), i64(B), i64(H), i64(W)) == 0, (S, B, H, W)


# ---- the patch -------------------------------------------------------------------------------------------------------------------------------
def test_patch_reference_reports_the_new_names():
    import test_patch_reference as TP
    if not os.path.isdir(os.path.join(TP.REFERENCE, "macarons")):
        pytest.skip("needs the MACARONS reference source tree, which is not part of this repository")
    TP._run("""
    import macarons.utility.macarons_utils as ref
    ref_tab, ref_fn = ref.regularity_tab, ref.get_regularity_loss_fn
    assert not hasattr(ref, "depth_scale_losses")
    import macarons_amd
    from macarons_amd.utility import macarons_utils as mu
    rep = macarons_amd.patch_reference(helpers="all")
    assert ref.depth_scale_losses is mu.depth_scale_losses
    assert ref.regularity_tab is mu.regularity_tab and ref.get_regularity_loss_fn is mu.get_regularity_loss_fn
    for name in ("depth_scale_losses", "regularity_tab", "get_regularity_loss_fn"):
        assert ("macarons.utility.macarons_utils", name) in rep["helpers"], name
    import macarons.utility.depth_model_utils as dmu
    assert dmu.regularity_tab is ref_tab and dmu.get_regularity_loss_fn is ref_fn      # the definitions are not touched
    from macarons_amd.patch import unpatch_reference
    unpatch_reference()
    assert ref.regularity_tab is ref_tab and ref.get_regularity_loss_fn is ref_fn and not hasattr(ref, "depth_scale_losses")
    print("__OK__")
    """)


def test_patch_lists_the_new_names():
    from macarons_amd import patch
    for name in ("get_regularity_loss_fn", "regularity_tab"):
        assert name in patch._HELPERS_ALL["utility.macarons_utils"][1] and name not in patch._HELPERS["utility.macarons_utils"][1]
    assert "depth_scale_losses" in patch._ADDITIONS_ALL["utility.macarons_utils"][1]


# ---- the cases at the kernels' edges (tests/_depth_loss_cases.py): what they reach, their conditions, and the reference itself -------------
import _depth_loss_cases as edge                                       # noqa: E402


def test_edge_cases_reach_what_they_are_for():
    """The sizes in the kernels' own numbers, so that a later change of DS_T, DS_MAX_S or the ratios cannot silently empty a case."""
    D = edge.DISPARITY
    assert len(D["s8"]["ratios"]) == ops.DISPARITY_MAX_SCALES == 8 and D["s8"]["ratios"].count(16) == 2 and D["s8"]["ratios"].count(1) == 2
    assert max(ops.DISPARITY_SCALE_RATIOS) == 16 and edge.n_tiles(D["s8"]["H"], D["s8"]["W"]) == 6 and D["s8"]["B"] == 2
    assert D["r16row"]["H"] // max(D["r16row"]["ratios"]) == 1                                # H_s = 1
    assert D["coarse0"]["ratios"][0] == 16 and 1 in D["coarse0"]["ratios"][1:]
    H, W = D["tiles65"]["H"], D["tiles65"]["W"]
    assert edge.cdiv(H, 16) * edge.cdiv(W, 16) > 64 and edge.n_tiles(H, W) > edge.FINISH_LANES and D["tiles65"]["B"] > 1
    assert 16 in D["tiles65"]["ratios"] and 16 in D["flat"]["ratios"]
    for tag in edge.DISPARITY_TAGS:                                      # every case is one the entry takes
        inp = edge.disparity_inputs(tag)
        assert len(inp["disps"]) <= ops.DISPARITY_MAX_SCALES
        assert all(D[tag]["H"] // d.shape[1] in ops.DISPARITY_SCALE_RATIOS and d.shape[1] * r == D[tag]["H"] and d.shape[2] * r == D[tag]["W"]
                   for d, r in zip(inp["disps"], D[tag]["ratios"]))
    s8 = edge.disparity_inputs("s8")["disps"]
    assert not np.array_equal(s8[0], s8[1]) and not np.array_equal(s8[2], s8[3]) and not np.array_equal(s8[6], s8[7])
    flat = edge.disparity_inputs("flat")["disps"]
    assert all(bool((d[0] == np.float32(edge.FLAT_VALUE)).all()) and bool((d[1] == 0).all()) for d in flat)


@pytest.mark.parametrize("tag,masked", edge.DISPARITY_VARIANTS)
def test_edge_conditions_and_composite_fp64_matches_model(tag, masked):
    """The golden generator's own conditions on the inputs, from the model alone (flat, whose differences are all exactly 0, is held
    to the second only): a least pair gap of 1e-4, at most 1 % of an image's pixels undecided, both values in every error mask.  And
    the check that the reference is right at the new shapes, for which there is no golden: the composite in fp64 against the model,
    which state the same mathematics with no shared code: 1e-9, the bound tests/test_reconstruction_loss_cpu.py uses for the same
    situation and far inside this file's TOL (measured: 1.8e-15 at most)."""
    inp = edge.disparity_inputs(tag)
    mask = inp["mask"] if masked else None
    gap, undecided_share, both, undecided = model.conditions(inp["disps"], inp["images"], mask)
    print(f"edge case {tag} mask={masked}: least pair gap {gap:.2e}; undecided {100 * undecided_share:.2f} %; both values {both}")
    assert undecided_share <= edge.MAX_UNDECIDED
    if tag != "flat":
        assert gap >= edge.MIN_GAP and both
    cr, g = edge.disparity_weights(tag)
    m = model.forward(inp["disps"], inp["images"], mask)
    ref = model.gradient(inp["disps"], inp["images"], mask, g, cr)
    depth, reg, em, tab, thr, grads = _composite(inp, masked, torch.float64, cr, g)
    e = dict(depth=model.rel(depth.detach(), m["depth"]), reg=model.rel(reg.detach(), m["reg"]), tab=model.rel(tab, m["tab"]),
             thr=model.rel(thr, m["thr"]), d_disp=max(model.rel(a, b) for a, b in zip(grads, ref)))
    print(f"edge case {tag} mask={masked}: composite fp64 vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < 1e-9 < TOL
    assert all(np.isfinite(r).all() for r in ref) and bool(((em.numpy() == m["error_mask"]) | undecided).all())
    if tag == "flat":                                                   # the exact zeros, in the model and in the composite
        assert (m["reg"] == 0).all() and (m["tab"] == 0).all() and (m["thr"] == 0).all() and not m["error_mask"].any()
        assert bool((reg == 0).all()) and bool((tab == 0).all()) and bool((thr == 0).all()) and not bool(em.any())
        assert all((r == 0).all() for r in model.gradient(inp["disps"], inp["images"], None, None, cr))
        assert m["depth"][:, 1].min() == m["depth"][:, 1].max() == model.ZFAR


def test_edge_coarse_scale_0_owns_the_table():
    """coarse0: the table, its threshold and the error mask come from scale 0, here the ratio-16 map, and are not those of the same
    maps with the full-resolution one first -- a test against this reference notices scale 0 being picked by resolution."""
    inp = edge.disparity_inputs("coarse0")
    m = model.forward(inp["disps"], inp["images"], inp["mask"])
    other = model.forward(edge.reordered(inp, (1, 0, 2))["disps"], inp["images"], inp["mask"])
    assert np.array_equal(m["depth"][[1, 0, 2]], other["depth"]) and np.array_equal(m["reg"][[1, 0, 2]], other["reg"])
    assert model.rel(m["tab"], other["tab"]) > 100 * TOL and model.rel(m["thr"], other["thr"]) > 100 * TOL
    decided = ~model.conditions(inp["disps"], inp["images"], inp["mask"])[3]
    assert ((m["error_mask"] != other["error_mask"]) & decided).sum() >= 16
