"""The reference-side binding (`macarons_amd.patch_reference`) exercised against the REAL reference.

Build-container only: /root/reference never travels to the GPU box, so these tests skip when it is absent.  Each scenario runs in
its own interpreter (the swap edits `sys.modules`; the rest of the suite must not see it).  PyTorch3D is absent here, so the
reference imports over the same stubs `tests/golden/_ref_import.py` gives the golden generator.

What "the drop-in is real" means here (Next #1):
  * `macarons/utility/scone_utils.py:13-14` and `macarons/networks/Macarons.py:5-6` import successfully and their
    `SconeOcc` / `SconeVis` / `KLDivCE` / `L1_loss` / `Uncentered_L1_loss` ARE the macarons_amd objects -- patch first or import first;
  * the reference's own weight-init walk (`scone_utils.py:260-428`), `initialize_scone_vis` (seed, init, optimiser), and its checkpoint
    loaders (`utils.py:140-185`, `Macarons.py:232-263`) run over the HIP classes and load reference-shaped checkpoints (with the DDP
    `module.` prefix);
  * the reference's `Macarons` wrapper dispatches to them and keeps its error strings;
  * the three training losses equal the reference's on random inputs.
"""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "macarons")),
                                     reason="needs the MACARONS reference source tree, which is not part of this repository")

PRELUDE = f"""
import sys, os, io, contextlib, importlib
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests", "golden"))
import _ref_import
_ref_import.install_stubs()            # pytorch3d / torchvision / matplotlib stand-ins + /root/reference on sys.path, no bytecode
import torch
import macarons_amd
hip = {{k: importlib.import_module("macarons_amd.networks." + k) for k in ("Attention", "SconeVis", "SconeOcc")}}
quiet = lambda: contextlib.redirect_stdout(io.StringIO())
"""


def _run(body):
    code = PRELUDE + textwrap.dedent(body) + "\nprint('__OK__')\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "__OK__" in r.stdout, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


@needs_reference
def test_patch_then_import():
    """The documented order: patch, then import the reference."""
    _run("""
    rep = macarons_amd.patch_reference()
    su = importlib.import_module("macarons.utility.scone_utils")          # scone_utils.py:13-14
    mac = importlib.import_module("macarons.networks.Macarons")           # Macarons.py:5-6
    for m in (su, mac):
        assert m.SconeOcc is hip["SconeOcc"].SconeOcc and m.SconeVis is hip["SconeVis"].SconeVis, m
    for n in ("KLDivCE", "L1_loss", "Uncentered_L1_loss"):
        assert getattr(su, n) is getattr(hip["SconeVis"], n), n
    assert sys.modules["macarons.networks.SconeVis"] is hip["SconeVis"]
    import macarons.networks
    assert macarons.networks.SconeOcc is hip["SconeOcc"]                  # attribute of the package = the MODULE
    from macarons.networks.SconeVis import SconeVis, KLDivCE, L1_loss, Uncentered_L1_loss     # the literal import line
    from macarons.networks.SconeOcc import SconeOcc
    assert SconeVis is hip["SconeVis"].SconeVis and SconeOcc is hip["SconeOcc"].SconeOcc
    # helpers either side of the networks
    mine = importlib.import_module("macarons_amd.utility.scone_utils")
    for n in ("compute_view_state", "move_view_state_to_view_space", "compute_view_harmonics", "compute_occupancy_probability",
              "filter_proxy_points", "sample_proxy_points"):
        assert getattr(su, n) is getattr(mine, n), n
        assert ("macarons.utility.scone_utils", n) in rep["helpers"]
    ru = importlib.import_module("macarons.utility.utils")
    assert ru.get_knn_points is importlib.import_module("macarons_amd.utility.utils").get_knn_points
    # every public name the reference's three modules define or hand on through `import *` resolves on ours
    # (knn_points: PyTorch3D's search, only reached with k_for_knn > 0, which no call site uses)
    assert rep["modules"] == ["macarons.networks.Attention", "macarons.networks.SconeVis", "macarons.networks.SconeOcc"]
    # idempotent
    rep2 = macarons_amd.patch_reference()
    assert su.SconeOcc is hip["SconeOcc"].SconeOcc and rep2["modules"] == rep["modules"]
    """)


@needs_reference
def test_import_then_patch_rebinds():
    """A process that imported the reference before patching: names already bound by `from ... import` are rebound."""
    _run("""
    su = importlib.import_module("macarons.utility.scone_utils")
    mac = importlib.import_module("macarons.networks.Macarons")
    mu = importlib.import_module("macarons.utility.macarons_utils")       # `from .scone_utils import *` etc.
    ref_vis_mod = sys.modules["macarons.networks.SconeVis"]
    ref_names = {k: sorted(n for n in dir(sys.modules["macarons.networks." + k]) if not n.startswith("_"))
                 for k in ("Attention", "SconeVis", "SconeOcc")}
    assert su.SconeVis is ref_vis_mod.SconeVis and su.SconeVis is not hip["SconeVis"].SconeVis
    ref_sample = su.sample_proxy_points
    rep = macarons_amd.patch_reference()
    for m in (su, mac, mu):
        for n in ("SconeOcc", "SconeVis"):
            if hasattr(m, n):
                assert getattr(m, n) is getattr(hip[n], n), (m.__name__, n)
    assert su.KLDivCE is hip["SconeVis"].KLDivCE and mac.Encoder is hip["Attention"].Encoder
    assert ("macarons.utility.scone_utils", "SconeVis") in rep["rebound"]
    assert su.sample_proxy_points is not ref_sample and mu.sample_proxy_points is su.sample_proxy_points
    # public-name coverage of the three modules: everything the reference exposes exists on ours, except PyTorch3D's knn_points
    for k, names in ref_names.items():
        missing = [n for n in names if not hasattr(hip[k], n)]
        assert missing in ([], ["knn_points"]), (k, missing)
    # upstream's Macarons class keeps its definition; its private copy of the scorer is routed to the HIP one
    from macarons_amd.networks.Macarons import Macarons as HipMacarons
    assert mac.Macarons is not HipMacarons
    assert mac.Macarons.compute_visibility_gains is HipMacarons.compute_visibility_gains
    macarons_amd.unpatch_reference()
    assert sys.modules["macarons.networks.SconeVis"] is ref_vis_mod and su.sample_proxy_points is ref_sample
    """)


@needs_reference
def test_reference_init_walk_optimiser_and_checkpoints_over_the_hip_classes(tmp_path):
    _run(f"""
    TMP = {str(tmp_path)!r}
    macarons_amd.patch_reference()
    su = importlib.import_module("macarons.utility.scone_utils")
    mac = importlib.import_module("macarons.networks.Macarons")
    ru = importlib.import_module("macarons.utility.utils")
    with quiet():
        vis, occ = su.SconeVis(use_sigmoid=True), su.SconeOcc()
    assert len(vis.state_dict()) == 60 and len(occ.state_dict()) == 172            # SURVEY 8b
    # (1) the reference's weight-init walks (named_modules -> nn.Linear children, last name component in w_q / w_k / w_v)
    before = {{k: v.clone() for k, v in vis.state_dict().items()}}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        torch.manual_seed(7)
        su.initialize_scone_vis_weights(vis)
        su.initialize_scone_occ_weights(occ)
    log = buf.getvalue()
    assert "encoders.0.mhsa.w_q initialized with Xavier normal." in log and "fc1 initialized with Kaiming normal." in log
    assert "local_transformers.2.encoders.1.mhsa.w_v initialized with Xavier normal." in log
    n_linear = sum(isinstance(m, torch.nn.Linear) for m in vis.modules()) + sum(isinstance(m, torch.nn.Linear) for m in occ.modules())
    assert log.count("initialized with") == n_linear
    assert not torch.equal(before["fc1.weight"], vis.state_dict()["fc1.weight"])
    # (2) initialize_scone_vis: seed + init + the reference's WarmupConstantOpt(AdamW) over our parameters
    class P:
        scone_vis_model_name = "t"; scone_occ_model_name = "t"; ddp = False; jz = False; learning_rate = 1e-4; warmup = 10; noam_opt = False
    with quiet():
        vis2, opt, opt_name, start_epoch, best_loss, best_cov = su.initialize_scone_vis(P, su.SconeVis(), "cpu", torch_seed=5)
        occ2, opt_o, _, _, _ = su.initialize_scone_occ(P, su.SconeOcc(), "cpu", torch_seed=5)
    assert opt_name == "WarmupAdamW" and start_epoch == 0 and isinstance(vis2, hip["SconeVis"].SconeVis)
    n_opt = sum(p.numel() for g in opt.optimizer.param_groups for p in g["params"])
    assert n_opt == sum(p.numel() for p in vis2.parameters()) == 1392888                 # SURVEY 8a6 [probe]
    assert sum(p.numel() for p in occ2.parameters()) == 2257769                        # SURVEY 8a7 [probe]
    # (3) reference-shaped checkpoints: DDP `module.` prefix through the reference's loaders
    ck_v = {{"epoch": 3, "loss": 0.5, "model_state_dict": {{"module." + k: v for k, v in vis.state_dict().items()}},
            "optimizer_state_dict": {{}}, "train_losses": [1.0], "val_losses": [1.0]}}
    ck_o = {{"epoch": 3, "loss": 0.5, "model_state_dict": dict(occ.state_dict())}}
    torch.save(ck_v, os.path.join(TMP, "vis.pth")); torch.save(ck_o, os.path.join(TMP, "occ.pth"))
    with quiet():
        v3 = ru.load_ddp_state_dict(su.SconeVis(), ck_v["model_state_dict"])               # utils.py:140-158
        v4 = mac.load_pretrained_module_weights_for_macarons(su.SconeVis(), os.path.join(TMP, "vis.pth"), True, "cpu")
        o4 = mac.load_pretrained_module_weights_for_macarons(su.SconeOcc(), os.path.join(TMP, "occ.pth"), False, "cpu")
    for k, v in vis.state_dict().items():
        assert torch.equal(v3.state_dict()[k], v) and torch.equal(v4.state_dict()[k], v), k
    for k, v in occ.state_dict().items():
        assert torch.equal(o4.state_dict()[k], v), k
    # (4) upstream's Macarons wrapper over the HIP modules: nested state dict keys, dispatch, error strings
    m = mac.Macarons(None, occ, vis)
    keys = list(m.state_dict())
    assert sum(k.startswith("occupancy.") for k in keys) == 172 and sum(k.startswith("visibility.") for k in keys) == 60
    try:
        m(mode="nope"); raise SystemExit("no error")
    except NameError as e:
        assert "Invalid mode" in str(e)
    try:
        m(mode="occupancy", proxy_points=torch.zeros(1, 4, 3)); raise SystemExit("no error")
    except NameError as e:
        assert "partial_point_cloud, proxy_points, view_harmonics" in str(e)
    # there is no CPU path: the HIP classes refuse CPU tensors loudly instead of computing something else
    try:
        m(mode="visibility", proxy_points=torch.zeros(1, 8, 4), view_harmonics=torch.zeros(1, 8, 64)); raise SystemExit("computed on CPU")
    except SystemExit:
        raise
    except Exception as e:
        assert "cuda" in str(e).lower() or "hip" in str(e).lower() or "device" in str(e).lower(), repr(e)
    """)


@needs_reference
def test_losses_equal_the_reference():
    _run("""
    ref = importlib.import_module("macarons.networks.SconeVis")           # the reference's own module (not patched here)
    assert ref is not hip["SconeVis"]
    g = torch.Generator().manual_seed(0)
    for shape in ((4, 52, 1), (1, 20, 1), (3, 7, 2)):
        x = torch.rand(shape, generator=g, dtype=torch.float64) + 0.05
        y = torch.rand(shape, generator=g, dtype=torch.float64) + 0.05
        for n in ("KLDivCE", "L1_loss", "Uncentered_L1_loss"):
            for dt in (torch.float64, torch.float32):
                xa = x.detach().clone().to(dt).requires_grad_(True); xb = x.detach().clone().to(dt).requires_grad_(True)
                a = getattr(ref, n)()(xa, y.to(dt)); b = getattr(hip["SconeVis"], n)()(xb, y.to(dt))
                tol = 1e-12 if dt == torch.float64 else 1e-6
                assert abs(float(a.detach()) - float(b.detach())) <= tol * max(1.0, abs(float(a))), (n, shape, float(a), float(b))
                a.backward(); b.backward()
                assert torch.allclose(xa.grad, xb.grad, rtol=1e-5 if dt == torch.float32 else 1e-10, atol=tol), (n, shape)
    """)


def test_losses_equal_the_reference_goldens():
    """The comparison above against the reference's recorded losses and gradients (tests/golden/reference_losses.npz, written by
    make_golden.py `losses` on the same inputs): runs without the reference tree."""
    import importlib
    import numpy as np
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    hip_vis = importlib.import_module("macarons_amd.networks.SconeVis")
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_losses.npz"))
    for si in range(3):
        x, y = torch.from_numpy(g[f"x{si}"]), torch.from_numpy(g[f"y{si}"])
        for n in ("KLDivCE", "L1_loss", "Uncentered_L1_loss"):
            for dt in (torch.float64, torch.float32):
                tag = f"{n}_{si}_{str(dt).split('.')[-1]}"
                a, a_grad = float(g[tag + "_loss"]), torch.from_numpy(g[tag + "_grad"])
                xb = x.detach().clone().to(dt).requires_grad_(True)
                b = getattr(hip_vis, n)()(xb, y.to(dt))
                tol = 1e-12 if dt == torch.float64 else 1e-6
                assert abs(a - float(b.detach())) <= tol * max(1.0, abs(a)), (n, si, a, float(b))
                b.backward()
                assert a_grad.dtype == xb.grad.dtype
                assert torch.allclose(a_grad, xb.grad, rtol=1e-5 if dt == torch.float32 else 1e-10, atol=tol), (n, si)


def test_integration_md_snippet_is_what_runs():
    """INTEGRATION.md §2 shows `macarons_amd.patch_reference()`; keep the document and the code from drifting apart."""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "macarons_amd.patch_reference()" in txt
    assert 'sys.modules["macarons.networks.SconeVis"] = _n.SconeVis' not in txt      # the round-4 alias installed a CLASS
