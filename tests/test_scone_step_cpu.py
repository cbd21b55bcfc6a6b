"""The online trainer's SCONE step without a GPU: the numpy restatement of the two K-frame kernels (tests/_frames_model.py) against the
golden the REFERENCE's memory_scene_loop produced (tests/golden/make_golden_scone_step.py), the loss helpers, and the host-side
refusal of a frame count outside 1 .. 32."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import golden

import _frames_cases as C
import _frames_model as M


@pytest.fixture(scope="module")
def step():
    g = golden("scone_step")
    return g, C.load_scone_step(g)


def test_model_reproduces_the_reference_signal(step):
    """Frustum masks, fov bits and the close mask (upstream's overwrite rule, then `out_of_field < 1`) exactly; signed distances within
    1e-5 (no recorded distance lies within 2e-3 of a threshold, so the masks cannot hang on that).  Measured: 9.5e-7 where |sgn| < 5,
    1.1e-3 = 2.0e-6 of the scale 549 overall."""
    g, s = step
    K, P = s["K"], s["P"]
    bits, sgn, close = M.supervision_frames(s["proxy"], s["recs"], s["depth"], s["dmask"], [1.1 * float(g["zfar"])] * K,
                                            float(g["surface_distance"]))
    for k in range(K):
        assert np.array_equal(((bits >> np.uint32(k)) & np.uint32(1)).astype(bool), s["fov_masks"][k]), f"frustum {k}"
    assert not s["fov_masks"][2].any() and int((s["fov_masks"][0] & s["fov_masks"][1]).sum()) > 100
    # within 1e-5 wherever the distance can decide anything (|sgn| < 5 holds every threshold: 1.5, 2.6, 0.05); a distance whose bilinear
    # footprint holds a masked pixel is a blend with the fill value 1.1 zfar = 550, where one fp32 ulp is already 6e-5 and the slope is
    # 540 per pixel: there the bound is 1e-5 of the scale
    err, mag = np.abs(sgn - g["sgn"]), np.abs(g["sgn"])
    scale = float(mag.max())
    e_near, e_all = float(err[mag < 5.].max()), float(err.max())
    print(f"ERR signed distances, model vs reference: {e_near:.2e} where |sgn| < 5, {e_all:.2e} = {e_all / scale:.2e} x the scale {scale:.1f} overall")
    assert int((mag < 5.).sum()) > 500 and e_near < 1e-5 and e_all < 1e-5 * scale
    assert np.array_equal(close & (s["before"]["oof"] < 1.), s["close_mask"])
    # the overwrite rule decides: a point both frames hold takes frame 1's test, and for some of them frame 0's test says otherwise
    both = s["fov_masks"][0] & s["fov_masks"][1]
    sd = np.float32(g["surface_distance"])
    differ = both & ((np.abs(sgn[0]) < sd) != (np.abs(sgn[1]) < sd))
    assert int(differ.sum()) == int(g["n_overwritten"]) > 0
    assert np.array_equal(close[differ], (np.abs(sgn[1]) < sd)[differ])


def test_model_reproduces_the_reference_state_tables(step):
    g, s = step
    b, a = s["before"], s["after"]
    bits = np.zeros(s["P"], np.uint32)
    for k in range(s["K"]):
        bits |= s["fov_masks"][k].astype(np.uint32) << np.uint32(k)
    vs, ni, nb, so, oof = M.update_frames(s["proxy"], bits, g["sgn"], s["eyes"], float(g["dts"]), float(g["carving_tolerance"]),
                                          float(g["score_threshold"]), 7, 14, b["view_states"], b["n_inside"], b["n_behind"], b["sup_occ"],
                                          b["oof"])
    assert b["n_inside"].max() >= 1 and not np.array_equal(a["view_states"], b["view_states"])
    assert np.array_equal(vs, a["view_states"])
    assert np.array_equal(ni, a["n_inside"]) and np.array_equal(nb, a["n_behind"])
    assert np.array_equal(so, a["sup_occ"]) and np.array_equal(oof, a["oof"])


def test_loss_helpers_follow_upstream():
    from macarons_amd.networks.SconeVis import KLDivCE, L1_loss, Uncentered_L1_loss
    from macarons_amd.utility import macarons_utils as mu
    assert type(mu.get_occ_loss_fn(NS(occ_loss_fn="mse"))) is torch.nn.MSELoss
    assert mu.get_occ_loss_fn(NS(occ_loss_fn="mse")).reduction == "mean"
    for name, cls in (("kl_divergence", KLDivCE), ("l1", L1_loss), ("uncentered_l1", Uncentered_L1_loss)):
        assert type(mu.get_cov_loss_fn(NS(cov_loss_fn=name))) is cls
    with pytest.raises(NameError, match="Invalid training loss function.Please choose a valid loss like 'mse'."):
        mu.get_occ_loss_fn(NS(occ_loss_fn="l2"))
    with pytest.raises(NameError, match="Please choose a valid loss between 'kl_divergence', 'l1' or 'uncentered_l1."):
        mu.get_cov_loss_fn(NS(cov_loss_fn="mse"))


@pytest.mark.parametrize("K", [0, 33])
def test_frame_counts_outside_1_to_32_are_refused_on_the_host(K):
    """Both the C entries (first check, before any pointer is looked at) and the wrappers (before any tensor is) refuse: no device."""
    from macarons_amd import _lib, ops
    from macarons_amd.utility import macarons_utils as mu
    L = _lib.lib()
    f = ctypes.c_float(1.0)
    rc = L.mcr_supervision_frames(None, ctypes.c_int64(5), None, ctypes.c_int(K), None, None, 2, 2, None, f, None, None, None, None)
    assert rc == 1 and b"between 1 and 32 frames" in L.mcr_last_error()
    rc = L.mcr_proxy_scene_update_frames(None, ctypes.c_int64(5), None, None, ctypes.c_int(K), None, f, f, f, 7, 14, None, None, None, None,
                                         None, None)
    assert rc == 1 and b"between 1 and 32 frames" in L.mcr_last_error()
    with pytest.raises(ValueError, match="between 1 and 32 frames"):
        ops.supervision_frames(torch.zeros(5, 3), torch.zeros(K, 40), torch.zeros(K, 2, 2), None, [1.0] * K, 1.0)
    with pytest.raises(ValueError, match="between 1 and 32 frames"):
        ops.proxy_scene_update_frames_(torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(K, 5), torch.zeros(K, 3), 1., 0., 1.,
                                       7, 14, *[torch.zeros(5, 1)] * 5)
    with pytest.raises(ValueError, match="between 1 and 32 frames"):
        mu.scone_supervision_step(None, None, None, None, [None] * K, None, None, None, 1.0, 1, None, None, "cpu")


def test_patch_reference_installs_the_step():
    """patch_reference(helpers="all") puts the loss helpers under upstream's names and ADDS the step and the batched clouds to the
    reference module (upstream writes them inline); the trainer module sees the helpers; unpatch takes the additions away again.
    Build container only (the reference tree does not travel); in its own interpreter, as tests/test_patch_reference.py."""
    import test_patch_reference as TP
    if not TP.os.path.isdir(TP.os.path.join(TP.REFERENCE, "macarons")):
        pytest.skip("needs the MACARONS reference source tree, which is not part of this repository")
    TP._run("""
    from macarons_amd.utility import macarons_utils as mu
    ref = importlib.import_module("macarons.utility.macarons_utils")
    tm = importlib.import_module("macarons.trainers.train_macarons")
    assert not hasattr(ref, "scone_supervision_step") and ref.get_cov_loss_fn is not mu.get_cov_loss_fn
    rep = macarons_amd.patch_reference(helpers="all")
    for n in ("get_occ_loss_fn", "get_cov_loss_fn", "scone_supervision_step", "compute_partial_point_clouds",
              "compute_occupancy_probability_for_supervision"):
        assert getattr(ref, n) is getattr(mu, n), n
        assert ("macarons.utility.macarons_utils", n) in rep["helpers"], n
    assert tm.get_occ_loss_fn is mu.get_occ_loss_fn and tm.get_cov_loss_fn is mu.get_cov_loss_fn       # `from ... import *` rebound
    from macarons_amd.patch import unpatch_reference
    unpatch_reference()
    assert not hasattr(ref, "scone_supervision_step") and not hasattr(ref, "compute_partial_point_clouds")
    assert ref.get_cov_loss_fn is not mu.get_cov_loss_fn and ref.get_cov_loss_fn.__module__ == "macarons.utility.macarons_utils"
    """)
