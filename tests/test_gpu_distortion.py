"""GPU: the distortion regulariser: the serial
reference-API op (raymarching.distortion_rays_train), the fused composite's
entries with the term (ngp_nerf_composite_loss_dist / _dist_lists),
FusedTrainer's and Trainer's dist_loss_weight, nerf.eval.ray_distortion and
main_nerf's flag.

The kernels are compared with distortion_helpers' float64 restatement of the
pairwise definition on its hand-built ray set (test_gpu_fused_depth.py's
loss_case, extended), with that file's bounds: per-ray values rtol 1e-4 /
atol 1e-5, gradients 1e-3 in the relative 2-norm, the whole step against
autograd 1e-3 (loss) and 1e-2 (parameter gradients)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import distortion_helpers as dh
from depth_helpers import write_scene

pytestmark = pytest.mark.gpu

N_RAYS = 1024
M_ROWS = 30000 + 128 - 30000 % 128
T_THRESH, SCALE = dh.T_THRESH, dh.SCALE


@pytest.fixture(scope="module")
def rs():
    return dh.ray_set()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    def make(name, *args, **kw):
        return write_scene(str(tmp_path_factory.mktemp(name)), *args, depth=False, **kw)
    return {"rgb32": make("rgb32", 6, 32, 32, channels=3), "lego32": make("lego32", 8, 32, 32, heldout=2)}


def _dataset(path, dev, store="uint8", type="train"):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, dev, type=type, scale=1.0, num_rays=N_RAYS, store=store)


def _model(dev):
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    with torch.no_grad():  # a non-trivial field: larger table values than the 1e-4 init
        model.encoder.embeddings.normal_(0, 0.05)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield(cascade=model.cascade, bound=1.0)).to(dev))
    return model


def _trainer(dev, data, seed=3, model=None, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(model if model is not None else _model(dev), data, M=M_ROWS, seed=seed, **kw)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def _nrel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run_entry(cuda, c, cw, dw, distw=None, live=False, lists=False, depth_job=True):
    """One launch on fresh buffers: the entry with the term (distw given) or
    the depth entry. depth_job False: the job with the colour-only defaults
    and no depth buffers (needs cw = 1, dw = 0)."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    N, M = c["N"], c["M"]
    d = {k: _dev(cuda, c[k]) for k in ("sigma", "col", "h", "deltas", "rays", "gt", "bg", "gtd")}
    half = lambda: torch.full((M, 16), 7.0, dtype=torch.float16, device=cuda)  # noqa: E731
    o = dict(g_col=half(), g_h=half(), loss=torch.full((N,), -1.0, device=cuda),
             dist=torch.full((N,), -1.0, device=cuda), depth=torch.full((N,), -1.0, device=cuda),
             ray_rows=torch.zeros(M, dtype=torch.int32, device=cuda), cnt=torch.zeros(N, dtype=torch.int32, device=cuda),
             rows=torch.full((M,), -1, dtype=torch.int32, device=cuda), total=torch.zeros(4, dtype=torch.int32, device=cuda))
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), SCALE, s), "fused_state_init")
    args = (P(d["sigma"]), P(d["col"]), P(d["h"]), P(d["deltas"]), P(d["rays"]), M, N, T_THRESH, 1.0, P(d["gt"]), 4,
            P(d["bg"]), P(state), P(o["g_col"]), P(o["g_h"]), None, None, P(o["loss"]))
    job = nat.DepthLossJob()
    job.color_weight, job.depth_weight, job.depth_min, job.depth_max = cw, dw, dh.LO, dh.HI
    if depth_job:
        job.gt_depth, job.out_depth = P(d["gtd"]), P(o["depth"])
    else:
        assert cw == 1.0 and dw == 0.0
    if live or lists:
        job.ray_rows, job.live_cnt = P(o["ray_rows"]), P(o["cnt"])
        if not lists:
            job.live_rows, job.live_total = P(o["rows"]), P(o["total"])
    if distw is None:
        entry = lib.ngp_nerf_composite_loss_depth_lists if lists else lib.ngp_nerf_composite_loss_depth
        nat.check(entry(*args, ctypes.byref(job), s), "composite_loss_depth")
    else:
        dj = nat.DistLossJob()
        dj.weight, dj.loss_dist_ray = distw, P(o["dist"])
        entry = lib.ngp_nerf_composite_loss_dist_lists if lists else lib.ngp_nerf_composite_loss_dist
        nat.check(entry(*args, ctypes.byref(job), ctypes.byref(dj), s), "composite_loss_dist")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _zero_rows(c):
    """Row ranges whose gradients must be exact zeros: behind the early stop, the overflow ray."""
    a = int(c["offs"][c["stop_ray"]])
    return [slice(a + 6, a + 96), slice(int(c["offs"][-1]), c["M"])]


# ---- 1. the serial op -------------------------------------------------------------------
def test_serial_op_matches_the_restatement(cuda, rs):
    import raymarching
    c = rs
    sigma = _dev(cuda, c["sigma"]).requires_grad_(True)
    dist = raymarching.distortion_rays_train(sigma, _dev(cuda, c["deltas"]), _dev(cuda, c["rays"]), T_THRESH)
    go = torch.linspace(0.5, 2.0, c["N"], device=cuda)  # by ray index
    dist.backward(go)
    torch.cuda.synchronize()
    got = dist.detach().cpu().numpy()[c["index"]]  # by list position
    gs = sigma.grad.cpu().numpy()
    want_gs = np.repeat(go.cpu().numpy().astype(np.float64)[c["index"]], c["counts"])[:c["M"]] * c["dsigma"]
    print(f"dist {got}\n want {c['dist']}\n grad rel {_nrel(gs, want_gs):.3e}")
    np.testing.assert_allclose(got, c["dist"], rtol=1e-4, atol=1e-5)
    assert (got[~c["valid"]] == 0).all() and (got[c["valid"]] > 0).all()
    assert np.abs(want_gs).max() > 0 and _nrel(gs, want_gs) <= 1e-3
    for z in _zero_rows(c):
        assert gs[z].size and (gs[z] == 0).all()


def test_serial_op_backward_is_the_derivative_of_its_forward(cuda):
    """gradcheck in fp32 on a 7-sample ray: central differences of the op's
    own forward, all 14 perturbed rays in one launch. eps = 2^-23. Step:
    h = sigma * eps^(1/3) (~0.5% of sigma), the usual balance of a central
    difference. Tolerance per component: a forward value f of 7 samples carries
    at most ~32 eps |f| of rounding (about ten rounded operations a sample and
    a 2-ulp expf feeding terms quadratic in w), so the difference quotient is
    off by at most 32 eps |f| / h; its truncation error is
    (h delta)^2 / 6 ~ 1e-6 relative; 1e-4 relative covers that and the
    backward's own fp32 rounding."""
    import raymarching
    rng = np.random.default_rng(11)
    n = 7
    deltas = np.stack([rng.uniform(0.003, 0.006, n), rng.uniform(0.001, 0.003, n)], -1).astype(np.float32)
    deltas[0, 1] = 0.3
    sigma = (rng.uniform(0.5, 1.5, n) * 3.0 / (n * 0.0045)).astype(np.float32)
    eps = 2.0 ** -23
    h = (sigma * eps ** (1 / 3)).astype(np.float32)
    R = 2 * n + 1
    sig = np.tile(sigma, (R, 1))
    for j in range(n):
        sig[1 + 2 * j, j] += h[j]
        sig[2 + 2 * j, j] -= h[j]
    rays = np.stack([np.arange(R), np.arange(R) * n, np.full(R, n)], -1).astype(np.int32)
    s = _dev(cuda, sig.reshape(-1)).requires_grad_(True)
    dist = raymarching.distortion_rays_train(s, _dev(cuda, np.tile(deltas, (R, 1))), _dev(cuda, rays), T_THRESH)
    dist[0].backward()
    torch.cuda.synchronize()
    f = dist.detach().cpu().numpy().astype(np.float64)
    got = s.grad.cpu().numpy()[:n].astype(np.float64)
    step = sig[1::2][np.arange(n), np.arange(n)].astype(np.float64) - sig[2::2][np.arange(n), np.arange(n)]
    fd = (f[1::2] - f[2::2]) / step
    tol = 32 * eps * f[0] / (step / 2) + 1e-4 * np.abs(got)
    print(f"f {f[0]:.6e}\n analytic {got}\n central  {fd}\n tol {tol}")
    assert (np.abs(got) > 10 * tol).sum() >= n - 1  # the check means something
    assert (np.abs(got - fd) <= tol).all()
    assert (s.grad.cpu().numpy()[n:] == 0).all()


# ---- 2. the fused entry -----------------------------------------------------------------
@pytest.mark.parametrize("cw,dw,distw", [(1.0, 0.0, 0.5), (1.0, 0.5, 0.5), (0.0, 0.0, 1.0)])
@pytest.mark.parametrize("live", [False, True])
def test_fused_entry_matches_the_reference_chain(cuda, rs, cw, dw, distw, live):
    c = rs
    want_loss, want_col, want_h0 = dh.loss_reference(c, cw, dw, distw)
    # (1, 0, .): the job with the colour-only defaults, the kernel without the depth form
    o = _run_entry(cuda, c, cw, dw, distw, live=live, depth_job=not (cw == 1.0 and dw == 0.0))
    g_col, g_h0 = o["g_col"].float().numpy(), o["g_h"][:, 0].float().numpy()
    for name, v in (("loss", o["loss"]), ("dist", o["dist"]), ("g_col", o["g_col"]), ("g_h", o["g_h"][:, 0])):
        assert torch.isfinite(v.float()).all(), name
    print(f"cw={cw} dw={dw} dist={distw} live={live}: dist {o['dist'].numpy()}\n  loss {o['loss'].numpy()}"
          f"\n  rel g_h {_nrel(g_h0, want_h0):.3e} g_col {_nrel(g_col, want_col):.3e}")
    np.testing.assert_allclose(o["dist"].numpy(), c["dist"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["loss"].numpy(), want_loss, rtol=1e-4, atol=1e-5)
    assert (o["dist"].numpy()[~c["valid"]].view(np.uint32) == 0).all()  # no composite: exactly +0
    assert np.abs(want_h0.astype(np.float64)).max() > 0
    assert _nrel(g_h0, want_h0) <= 1e-3
    if cw == 0.0:
        assert (g_col == 0).all()  # the distortion gradient alone
        # ... and it is there: the chain without the term gives no gradient at all
        assert (dh.loss_reference(c, cw, dw, 0.0)[2] == 0).all() and (g_h0 != 0).sum() > c["M"] // 2
    else:
        assert _nrel(g_col, want_col) <= 1e-3
    assert (o["g_col"][:, 3:] == 0).all()
    for z in _zero_rows(c):
        assert g_h0[z].size and (g_col[z] == 0).all() and (g_h0[z] == 0).all()
    if live:
        nz = np.flatnonzero((g_col != 0).any(1) | (g_h0 != 0))
        total = int(o["total"][0])
        assert total == nz.size > 0
        assert np.array_equal(o["rows"].numpy()[:total], nz)
        # the _lists form: the same per-ray lists and gradients, no joined list
        p = _run_entry(cuda, c, cw, dw, distw, lists=True, depth_job=not (cw == 1.0 and dw == 0.0))
        assert torch.equal(p["cnt"], o["cnt"]) and int(p["cnt"].sum()) == total
        for n, (a, k) in enumerate(zip(c["offs"], p["cnt"].numpy())):
            assert torch.equal(p["ray_rows"][a:a + k], o["ray_rows"][a:a + k]), n
        assert torch.equal(_bits(p["g_h"][:, 0]), _bits(o["g_h"][:, 0])) and torch.equal(_bits(p["loss"]), _bits(o["loss"]))
        assert int(p["total"][0]) == 0 and (p["rows"] == -1).all()


# ---- 3. weight 0 ------------------------------------------------------------------------
@pytest.mark.parametrize("live", [False, True])
def test_zero_weight_is_the_depth_entry_bit_for_bit(cuda, rs, live):
    c = rs
    a = _run_entry(cuda, c, 1.0, 0.5, 0.0, live=live)
    b = _run_entry(cuda, c, 1.0, 0.5, None, live=live)
    for name in ("loss", "g_col", "g_h", "depth"):
        va, vb = a[name], b[name]
        if name == "g_h":
            va, vb = va[:, 0], vb[:, 0]  # (the kernel writes column 0)
        assert torch.equal(_bits(va), _bits(vb)), name
    if live:
        total = int(b["total"][0])
        assert int(a["total"][0]) == total > 0
        assert torch.equal(a["rows"][:total], b["rows"][:total]) and torch.equal(a["cnt"], b["cnt"])
    # ... and the term is still reported
    np.testing.assert_allclose(a["dist"].numpy(), c["dist"], rtol=1e-4, atol=1e-5)
    assert (b["dist"] == -1).all()
    # the colour-only job at weight 0 (the kernel without the depth form): the same colour loss and gradients
    p = _run_entry(cuda, c, 1.0, 0.0, 0.0, live=live, depth_job=False)
    q = _run_entry(cuda, c, 1.0, 0.0, None, live=live, depth_job=False)
    for name in ("loss", "g_col", "g_h"):
        va, vb = (p[name], q[name]) if name != "g_h" else (p[name][:, 0], q[name][:, 0])
        assert torch.equal(_bits(va), _bits(vb)), name
    np.testing.assert_allclose(p["dist"].numpy(), c["dist"], rtol=1e-4, atol=1e-5)


# ---- 4. fused = serial ------------------------------------------------------------------
def test_fused_term_equals_the_serial_op(cuda, rs):
    import raymarching
    c = rs
    o = _run_entry(cuda, c, 1.0, 0.0, 0.5, depth_job=False)
    with torch.no_grad():
        serial = raymarching.distortion_rays_train(_dev(cuda, c["sigma"]), _dev(cuda, c["deltas"]),
                                                   _dev(cuda, c["rays"]), T_THRESH)
    serial = serial.cpu().numpy()[c["index"]]
    print(f"fused {o['dist'].numpy()}\nserial {serial}")
    np.testing.assert_allclose(o["dist"].numpy(), serial, rtol=1e-4, atol=1e-5)


# ---- 5. the whole step against autograd -------------------------------------------------
STEP_WEIGHT = 1.0


def test_dist_step_matches_autograd(cuda, scenes):
    """FusedTrainer._forward_backward against Trainer._forward_backward (the
    serial op through autograd) on the same batch, as
    test_gpu_fused_depth.py::test_depth_step_matches_autograd. RGB images: both
    blend on white. dist_loss_weight = STEP_WEIGHT = 1.0: on this random field
    the mean term is 0.0032 beside a colour loss of 0.038, and the step
    without the term has a table gradient 0.575 away from the reference's in
    the relative norm, against 6.9e-4 with it and a bound of 1e-2 (measured on
    an MI355X; the figures are printed)."""
    from nerf.train import Trainer
    w = STEP_WEIGHT
    data = _dataset(scenes["rgb32"], cuda)
    f32 = _dataset(scenes["rgb32"], cuda, store="float32")
    base = _model(cuda)
    ref, plain_model = copy.deepcopy(base), copy.deepcopy(base)
    ref.mean_count = 30000

    def fused(model, weight):
        ft = _trainer(cuda, data, model=model, dist_loss_weight=weight)
        ft._sample()
        ft.noises.zero_()  # the autograd step marches with perturb=False
        ft._forward_backward()
        torch.cuda.synchronize()
        return ft

    ft = fused(base, w)
    gt = f32.images[int(ft.image_index)].view(-1, 3)[ft.pix.long()]
    tr = Trainer(ref, data, dist_loss_weight=w, perturb=False, update_density=False)
    assert float(tr.scaler.get_scale()) == ft.scale
    batch = {"rays_o": ft.rays_o.clone()[None], "rays_d": ft.rays_d.clone()[None], "images": gt[None]}
    ref.train()
    loss = tr._forward_backward(batch)
    torch.cuda.synchronize()
    assert int(ft.counter[0]) == int(ref.step_counter[0, 0]) > 0
    fused_loss = float(ft.loss_ray.double().sum()) / ft.N
    fused_dist = float(ft.loss_dist_ray.double().sum()) / ft.N
    lv, dv = float(loss.detach()), float(tr.last_dist_loss)
    print(f"samples {int(ft.counter[0])} loss fused {fused_loss:.8f} autograd {lv:.8f}; dist term {fused_dist:.8f} "
          f"/ {dv:.8f}")
    assert abs(fused_loss - lv) <= 1e-3 * abs(lv) + 1e-7
    assert dv > 0 and abs(fused_dist - dv) <= 1e-3 * dv + 1e-7
    refs = [ref.encoder.embeddings.grad, ref.sigma_net.weights.grad, ref.color_net.weights.grad]
    for name, g, r in zip(["embeddings", "sigma_net", "color_net"], ft.grads, refs):
        print(f"grad {name} rel {_rel(g, r):.3e}")
        assert torch.isfinite(g.float()).all(), name
        assert r.abs().max() > 0, name
        assert _rel(g, r) < 1e-2, (name, _rel(g, r))
    # ... and the term is in that gradient: the step without it differs by more than the bound
    ft0 = fused(plain_model, 0.0)
    assert torch.equal(ft0.pix, ft.pix) and ft0._dist_job is None
    away = _rel(ft0.grads[0], refs[0])
    print(f"weight-0 embeddings grad rel {away:.3e}")
    assert away > 1e-2


# ---- 6. off is off ----------------------------------------------------------------------
def test_zero_weight_changes_nothing(cuda, scenes):
    """dist_loss_weight = 0 and a trainer built without the argument: the same
    launches, so 20 steps (eager, then captured) end bit-identical."""
    data = _dataset(scenes["lego32"], cuda)
    a, b = _trainer(cuda, data, dist_loss_weight=0.0), _trainer(cuda, data)
    assert a._dist_job is None and a.last_dist_loss is None and a.last_color_loss is None
    for ft in (a, b):
        for _ in range(8):
            ft.step()
        ft.capture()  # 2 more eager steps, then the graphs
        ft.run(10)
        ft.flush()
    torch.cuda.synchronize()
    assert a.optimizer_steps == b.optimizer_steps > 0
    assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))
    assert a.last_loss == b.last_loss and np.isfinite(a.last_loss)
    names = [list(t.timed_body_steps(1)[0]) for t in (a, b)]
    assert names[0] == names[1] and "composite_loss" in names[0]


# ---- 7. it regularises ------------------------------------------------------------------
def test_the_term_lowers_the_heldout_ray_distortion(cuda, scenes):
    """8 RGBA views at 32 x 32 and 2 the training never saw; the same seed and
    300 steps with and without the term. The engine is bit-reproducible, so
    the comparison is a fixed fact. No PSNR bound: the pair is printed."""
    from nerf.eval import psnr, ray_distortion
    data, val = _dataset(scenes["lego32"], cuda), _dataset(scenes["lego32"], cuda, type="val")
    assert data.poses.shape[0] == 8 and val.poses.shape[0] == 2
    out = {}
    for w in (0.0, 0.1):
        ft = _trainer(cuda, data, dist_loss_weight=w)
        for _ in range(4):
            ft.step()
        ft.capture()
        ft.run(294)
        ft.flush()
        torch.cuda.synchronize()
        assert ft.device_errors() == 0 and np.isfinite(ft.last_loss) and ft.sample_count() < ft.M
        rd = float(np.mean([ray_distortion(ft.model, val, i) for i in range(2)]))
        ps = float(np.mean([psnr(ft.model, val, i) for i in range(2)]))
        out[w] = (rd, ps)
        print(f"dist_loss_weight {w}: held-out ray distortion {rd:.6f}, PSNR {ps:.4f}, loss {ft.last_loss:.6f}, "
              f"dist term {ft.last_dist_loss}")
    assert np.isfinite(out[0.0][0]) and np.isfinite(out[0.1][0]) and out[0.0][0] > 0
    assert out[0.1][0] < out[0.0][0]


# ---- 8. main_nerf -----------------------------------------------------------------------
def test_main_nerf_trains_with_the_term_and_reports_it(cuda, scenes, tmp_path, capsys):
    import main_nerf
    args = ["-O", "--workspace", str(tmp_path / "ws"), "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--iters",
            "64", "--num_rays", "1024", "--sample_budget", "131072", "--dist_loss_weight", "0.1"]
    out = main_nerf.main([scenes["lego32"], *args])
    text = capsys.readouterr().out
    assert "PSNR" in text and "ray distortion" in text and "(rgb " in text and ", dist " in text
    assert "device errors 0" in text
    assert np.isfinite(out["psnr"]) and np.isfinite(out["loss"])
    assert out["dist_loss"] is not None and np.isfinite(out["dist_loss"]) and out["dist_loss"] >= 0
    assert out["ray_distortion"] is not None and np.isfinite(out["ray_distortion"]) and out["ray_distortion"] >= 0


# ---- 9. errors --------------------------------------------------------------------------
def test_argument_errors(cuda, scenes, rs):
    import _ngp_native as nat
    data = _dataset(scenes["lego32"], cuda)
    with pytest.raises(ValueError, match="dist_loss_weight"):
        _trainer(cuda, data, dist_loss_weight=-0.1)
    with pytest.raises(ValueError, match="dist_loss_weight is single-process only"):
        _trainer(cuda, data, dist_loss_weight=0.1, distributed=True)
    # a null dist job: NGP_ERR_ARG, nothing launched (the buffers keep their fill)
    lib = nat.lib()
    job = nat.DepthLossJob()
    job.color_weight = 1.0
    loss = torch.full((rs["N"],), -1.0, device=cuda)
    for entry in (lib.ngp_nerf_composite_loss_dist, lib.ngp_nerf_composite_loss_dist_lists):
        rc = entry(None, None, None, None, None, rs["M"], rs["N"], T_THRESH, 1.0, None, 4, None, None, None, None,
                   None, None, nat.ptr(loss), ctypes.byref(job), None, None)
        assert rc == -1 and b"dist job" in lib.ngp_last_error()
    torch.cuda.synchronize()
    assert (loss == -1).all()
