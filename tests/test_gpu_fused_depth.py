"""GPU: depth-supervised training on the fused engine: the device depth gather
beside the pixel gather (ngp_image_source's depth stack), the depth form of
the composite + loss kernel (ngp_nerf_composite_loss_depth), FusedTrainer's
and Trainer's loss weights, nerf.eval.depth_error and main_nerf's flags.

The scenes are written by depth_helpers: the Lego boxes' images with one
depth_k.npz per frame, the analytic distance to the nearest box (0 on a miss)
in the poses' units. The cameras stand ~3.2 from the origin, outside the
bound-1 box, so the bound-1 tests load the maps with depth_scale 0.25: the
targets then lie inside the loss's mask [min_near, bound] = [0.2, 1]."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from depth_helpers import write_scene

pytestmark = pytest.mark.gpu

N_RAYS = 1024
M_ROWS = 30000 + 128 - 30000 % 128
DEPTH_SCALE = 0.25


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """The module's scenes, written once."""
    def make(name, *args, **kw):
        return write_scene(str(tmp_path_factory.mktemp(name)), *args, **kw)
    return {"colmap": make("colmap", 5, 24, 40, colmap=True),
            "lego32": make("lego32", 6, 32, 32),
            "lego32_plain": make("lego32_plain", 6, 32, 32, depth=False),
            "rgb32": make("rgb32", 6, 32, 32, channels=3),
            "lego64": make("lego64", 8, 64, 64, heldout=1)}


def _dataset(path, dev, store="uint8", type="train", scale=1.0, depth_scale=DEPTH_SCALE):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, dev, type=type, scale=scale, num_rays=N_RAYS, store=store, depth_scale=depth_scale)


def _model(dev, bound=1, bits=None, **kw):
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=bound, cuda_ray=True, density_thresh=10, **kw).to(dev)
    with torch.no_grad():  # a non-trivial field: larger table values than the 1e-4 init
        model.encoder.embeddings.normal_(0, 0.05)
    bits = bits if bits is not None else lego_bitfield(cascade=model.cascade, bound=float(bound))
    model.density_bitfield.copy_(torch.from_numpy(bits).to(dev))
    return model


def _trainer(dev, data, seed=3, options=None, model=None, M=M_ROWS, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(model if model is not None else _model(dev), data, M=M, seed=seed, options=options, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def _want_depth(data, ft):
    return data.depths[int(ft.image_index)].view(-1)[ft.pix.long()] * data.depth_scale


# ---- 1. the gather ------------------------------------------------------------------
def test_gather(cuda, scenes):
    """Ray n's target depth is its pixel of the drawn image's depth map times
    depth_scale (fx != fy, off-centre principal point, H != W); everything
    else of the draw is the colour-only draw's, bit for bit."""
    import _ngp_native as nat
    data = _dataset(scenes["colmap"], cuda)
    assert data.depths.shape == (5, 24, 40) and data.depth_scale == DEPTH_SCALE
    assert data.intrinsics[0] != data.intrinsics[1] and data.intrinsics[2] != 40 / 2
    ft = _trainer(cuda, data, depth_loss_weight=0.5)
    plain = _trainer(cuda, data)  # default weights: the colour-only draw, no depth source
    assert ft._depth and ft._src.depths and not plain._depth and not plain._src.depths
    for draw in range(2):
        ft._sample()
        plain._sample()
        torch.cuda.synchronize()
        want = _want_depth(data, ft)
        assert torch.equal(_bits(ft.gt_depth), _bits(want)), draw
        hit = want > 0
        assert N_RAYS // 50 < int(hit.sum()) < N_RAYS  # boxes and background both drawn
        assert 0.2 < float(want[hit].min()) and float(want.max()) < 1.0  # inside the mask
        for name in ("rgba", "rays_o", "rays_d", "bg", "nears", "fars", "noises", "pix", "image_index"):
            assert torch.equal(_bits(getattr(ft, name)), _bits(getattr(plain, name))), (draw, name)
    # ngp_image_rays with the depth stack, on its own buffers and a fresh state: draw 0 again
    ft = _trainer(cuda, data, depth_loss_weight=0.5)
    ft._sample()
    lib, P, N = nat.lib(), nat.ptr, N_RAYS
    f = {k: torch.zeros(N, w, device=cuda) for k, w in (("rays_o", 3), ("rays_d", 3), ("rgba", 4), ("bg", 3))}
    f.update({k: torch.zeros(N, device=cuda) for k in ("nears", "fars", "noises")})
    pix = torch.full((N,), -1, dtype=torch.int32, device=cuda)
    index = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    depth = torch.full((N,), -1.0, device=cuda)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), 65536.0, s), "fused_state_init")
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = P(data.images), 4, nat.DTYPE_U8
    src.pix, src.image_index = P(pix), P(index)
    src.depths, src.depth_scale, src.depth_out = P(data.depths), DEPTH_SCALE, P(depth)
    nat.check(lib.ngp_image_rays(P(data.poses), data.poses.shape[0], ft._intr, data.H, data.W, N, ctypes.byref(src),
                                 ft._aabb, float(ft.model.min_near), ft.seed, P(state), P(f["rays_o"]),
                                 P(f["rays_d"]), P(f["rgba"]), P(f["bg"]), P(f["nears"]), P(f["fars"]),
                                 P(f["noises"]), P(counter), None, s), "image_rays")
    torch.cuda.synchronize()
    assert torch.equal(pix, ft.pix) and torch.equal(_bits(f["rgba"]), _bits(ft.rgba))
    assert torch.equal(_bits(depth), _bits(ft.gt_depth))


@pytest.mark.parametrize("live", [True, False])
def test_both_draw_sites_gather_the_same_depths(cuda, scenes, live):
    """The draw in the grid backward's bin launch (draw_ahead, over the live
    rows or all rows) against the draw in the head launch: after step i the
    draw-ahead trainer holds batch i + 1, the other batch i (as
    test_gpu_fused_images.py::test_both_draw_sites_draw_the_same_batches)."""
    data = _dataset(scenes["lego32"], cuda)
    a = _trainer(cuda, data, options=dict(live_rows=live), depth_loss_weight=0.5)
    b = _trainer(cuda, data, options=dict(live_rows=live, draw_ahead=False), depth_loss_weight=0.5)
    assert a._draw_ahead and a._live == live and not b._draw_ahead
    batches = []
    for i in range(4):
        if i < 3:
            a.step()
        b.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(b.gt_depth), _bits(_want_depth(data, b))), i
        if i > 0:  # b holds batch i, which a drew during step i - 1
            pa, da = batches[i - 1]
            assert torch.equal(pa, b.pix) and torch.equal(_bits(da), _bits(b.gt_depth)), i
        if i < 3:
            assert a._ahead
            assert torch.equal(_bits(a.gt_depth), _bits(_want_depth(data, a))), i
            batches.append((a.pix.clone(), a.gt_depth.clone()))
            la, lb, da_, db_ = a.last_loss, b.last_loss, a.last_depth_loss, b.last_depth_loss
            print(f"live={live} step {i}: loss {la!r} / {lb!r}, depth term {da_!r} / {db_!r}")
            assert a.sample_count() == b.sample_count() > 0, i
            assert la == lb and np.isfinite(la) and da_ == db_ and da_ > 0, (i, la, lb, da_, db_)


def test_depth_weight_needs_depth_maps(cuda, scenes):
    from nerf.provider import SyntheticLego
    with pytest.raises(ValueError, match="depth_loss_weight"):
        _trainer(cuda, _dataset(scenes["lego32_plain"], cuda), depth_loss_weight=0.5)
    with pytest.raises(ValueError, match="depth_loss_weight"):
        _trainer(cuda, SyntheticLego(cuda, num_rays=N_RAYS), depth_loss_weight=0.5)
    # a draw site without an image (and so without a depth) form: the existing error
    with pytest.raises(ValueError, match="march_adam"):
        _trainer(cuda, _dataset(scenes["lego32"], cuda), options=dict(march_adam=False), depth_loss_weight=0.5)


# ---- 2. the loss kernel against the serial reference --------------------------------
COUNTS = [0, 1, 63, 64, 65, 128, 255, 256, 257, 320, 96, 80]
LO, HI, T_THRESH, SCALE = 0.2, 1.0, 1e-4, 65536.0


@pytest.fixture(scope="module")
def loss_case():
    """Hand-built inputs hitting every path of k_composite_loss, and the serial
    reference's forward (oracle, CPU), shared by the weightings.
    12 rays of COUNTS samples: 0 (no samples); 64/65 the wave boundary; 256/257
    the boundary between the kept chunks (kLossPre = 4) and the reloaded ones;
    the 96-sample ray has sigma 1e9 at its sample 5 and stops there; the
    80-sample ray overflows M. Each ray's sigma * delta sums to ~3 (no other ray
    stops early), and its first delta-t is 0.3, so every depth is above LO."""
    import oracle
    rng = np.random.default_rng(17)
    N = len(COUNTS)
    offs = np.concatenate([[0], np.cumsum(COUNTS)[:-1]]).astype(np.int64)
    M = int(offs[-1]) + 40  # the last ray's 80 rows do not fit
    index = rng.permutation(N)  # the ray index is not the list position
    rays = np.stack([index, offs, COUNTS], -1).astype(np.int32)
    d0 = rng.uniform(0.003, 0.006, M).astype(np.float32)
    d1 = rng.uniform(0.001, 0.003, M).astype(np.float32)
    sigma = np.zeros(M, np.float32)
    for n, (o, c) in enumerate(zip(offs, COUNTS)):
        e = min(o + c, M)
        if c:
            d1[o] = 0.3
            sigma[o:e] = rng.uniform(0.5, 1.5, e - o) * 3.0 / (c * 0.0045)
    stop_ray = COUNTS.index(96)
    sigma[offs[stop_ray] + 5] = 1e9
    deltas = np.stack([d0, d1], -1)
    col = rng.normal(0, 2, (M, 16)).astype(np.float16)
    h = rng.normal(0, 1, (M, 16)).astype(np.float16)
    gt = rng.uniform(0, 1, (N, 4)).astype(np.float32)
    bg = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    rgbs = (1 / (1 + np.exp(-col[:, :3].astype(np.float32)))).astype(np.float16).astype(np.float32)
    ws, dp, img = oracle.composite_rays_train_forward(sigma, rgbs, deltas, rays, T_THRESH)
    pred = dp[index]  # by list position
    valid = np.array([c > 0 and o + c <= M for o, c in zip(offs, COUNTS)])
    assert (pred[valid] > 0).all() and (pred[~valid] == 0).all()
    # the targets, by list position: in the mask above / below the depth, below
    # min_near, above bound, 0, NaN; the no-sample and the overflow ray in the mask
    kind = ["in", "above", "below", "low", "high", "zero", "nan", "above", "below", "above", "above", "in"]
    val = {"in": 0.5, "low": 0.1, "high": 1.5, "zero": 0.0, "nan": np.nan}
    gtd_n = np.array([pred[n] + 0.25 if k == "above" else pred[n] - 0.05 if k == "below" else val[k]
                      for n, k in enumerate(kind)], np.float32)
    masked = np.array([k in ("low", "high", "zero", "nan") for k in kind])
    assert (gtd_n[~masked] >= LO + 0.01).all() and (gtd_n[~masked] <= HI - 0.01).all()  # well inside the mask
    gtd = np.zeros(N, np.float32)
    gtd[index] = gtd_n  # the kernel reads the target by ray index
    return dict(N=N, M=M, rays=rays, index=index, offs=offs, sigma=sigma, deltas=deltas, col=col, h=h, gt=gt, bg=bg,
                rgbs=rgbs, ws=ws, dp=dp, img=img, gtd=gtd, gtd_n=gtd_n, masked=masked, valid=valid,
                stop_ray=stop_ray)


def _loss_reference(c, cw, dw):
    """loss_ray, loss_depth_ray and the fp16 gradients the reference chain
    gives: oracle composite backward with grad_depth, then rgbs.float() <- half
    and sigmoid backward, and sigmas = trunc_exp(h0) backward, in numpy."""
    import oracle
    N, index = c["N"], c["index"]
    f32 = np.float32
    # by ray index, as the reference's [N] tensors
    p = c["img"] + (1 - c["ws"])[:, None] * c["bg"]
    a = c["gt"][:, 3:]
    q = c["gt"][:, :3] * a + c["bg"] * (1 - a)
    e = (p - q).astype(f32)
    mse = ((e * e).sum(-1) / 3).astype(f32)
    pred = np.maximum(c["dp"], 0)
    with np.errstate(invalid="ignore"):
        mask = (LO <= c["gtd"]) & (c["gtd"] <= HI)
        dep = np.where(mask, np.abs(c["gtd"] - pred), 0).astype(f32)
        sgn = np.where(mask, np.sign(pred - c["gtd"]), 0).astype(f32)
    loss = (cw * mse + dw * dep).astype(f32)
    g_img = (f32(SCALE * cw / N / 3) * 2 * e).astype(f32)
    g_ws = -(g_img * c["bg"]).sum(-1).astype(f32)
    g_dep = (f32(SCALE * dw / N) * sgn).astype(f32)
    gs, gc = oracle.composite_rays_train_backward(g_ws, g_dep, g_img, c["sigma"], c["rgbs"], c["deltas"], c["rays"],
                                                  c["ws"], c["dp"], c["img"], T_THRESH)
    y = c["rgbs"]
    g_col = np.zeros((c["M"], 16), np.float16)
    with np.errstate(over="ignore"):
        g_col[:, :3] = (gc.astype(np.float16).astype(f32) * (1 - y) * y).astype(np.float16)
        g_h0 = (gs * np.exp(np.clip(c["h"][:, 0].astype(f32), -15, 15))).astype(np.float16)
    return loss[index], dep[index], g_col, g_h0  # the per-ray outputs by list position


def _run_loss(cuda, c, cw=None, dw=None, live=False):
    """One launch on fresh buffers: the depth entry (cw, dw given) or the
    colour-only entries."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    N, M = c["N"], c["M"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    d = dict(sigma=t(c["sigma"]), col=t(c["col"]), h=t(c["h"]), deltas=t(c["deltas"]), rays=t(c["rays"]),
             gt=t(c["gt"]), bg=t(c["bg"]), gtd=t(c["gtd"]))
    half = lambda: torch.full((M, 16), 7.0, dtype=torch.float16, device=cuda)  # noqa: E731
    o = dict(g_col=half(), g_h=half(), loss=torch.full((N,), -1.0, device=cuda),
             depth=torch.full((N,), -1.0, device=cuda), dep=torch.full((N,), -1.0, device=cuda),
             ray_rows=torch.zeros(M, dtype=torch.int32, device=cuda), cnt=torch.zeros(N, dtype=torch.int32, device=cuda),
             rows=torch.full((M,), -1, dtype=torch.int32, device=cuda), total=torch.zeros(4, dtype=torch.int32, device=cuda))
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), SCALE, s), "fused_state_init")
    args = (P(d["sigma"]), P(d["col"]), P(d["h"]), P(d["deltas"]), P(d["rays"]), M, N, T_THRESH, 1.0, P(d["gt"]), 4,
            P(d["bg"]), P(state), P(o["g_col"]), P(o["g_h"]), None, None, P(o["loss"]))
    lists = (P(o["ray_rows"]), P(o["cnt"]), P(o["rows"]), P(o["total"]))
    if cw is None:
        if live:
            nat.check(lib.ngp_nerf_composite_loss_live(*args, *lists, s), "composite_loss_live")
        else:
            nat.check(lib.ngp_nerf_composite_loss(*args, s), "composite_loss")
    else:
        job = nat.DepthLossJob()
        job.gt_depth, job.color_weight, job.depth_weight, job.depth_min, job.depth_max = P(d["gtd"]), cw, dw, LO, HI
        job.out_depth, job.loss_depth_ray = P(o["depth"]), P(o["dep"])
        if live:
            job.ray_rows, job.live_cnt, job.live_rows, job.live_total = lists
        nat.check(lib.ngp_nerf_composite_loss_depth(*args, ctypes.byref(job), s), "composite_loss_depth")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _nrel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


@pytest.mark.parametrize("cw,dw", [(1.0, 0.5), (0.0, 1.0)])
@pytest.mark.parametrize("live", [False, True])
def test_loss_kernel_matches_the_serial_reference(cuda, loss_case, cw, dw, live):
    c = loss_case
    want_loss, want_dep, want_col, want_h0 = _loss_reference(c, cw, dw)
    o = _run_loss(cuda, c, cw, dw, live=live)
    g_col, g_h0 = o["g_col"].float().numpy(), o["g_h"][:, 0].float().numpy()
    depth = o["depth"].numpy()[c["index"]]  # by list position
    for name, v in (("loss", o["loss"]), ("dep", o["dep"]), ("depth", o["depth"]), ("g_col", o["g_col"]),
                    ("g_h", o["g_h"][:, 0])):
        assert torch.isfinite(v.float()).all(), name
    print(f"cw={cw} dw={dw} live={live}: depth {depth}\n  dep {o['dep'].numpy()}\n  loss {o['loss'].numpy()}"
          f"\n  rel g_h {_nrel(g_h0, want_h0):.3e} g_col {_nrel(g_col, want_col):.3e}")
    # the fused composite's bound (test_gpu_fused.py test_composite_loss_large_densities_match_serial)
    np.testing.assert_allclose(depth, c["dp"][c["index"]], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["loss"].numpy(), want_loss, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o["dep"].numpy(), want_dep, rtol=1e-4, atol=1e-5)
    # masked-out targets (below min_near, above bound, 0, NaN): exactly +0
    assert (o["dep"].numpy()[c["masked"]].view(np.uint32) == 0).all()
    assert (o["dep"].numpy()[~c["masked"]] > 0.04).all()
    # the rays without a composite compare their target to a depth of 0
    assert np.array_equal(o["dep"].numpy()[~c["valid"]], c["gtd_n"][~c["valid"]]) and (depth[~c["valid"]] == 0).all()
    # gradients: the end-to-end bound
    assert np.abs(want_h0.astype(np.float64)).max() > 0
    assert _nrel(g_h0, want_h0) <= 1e-3
    if cw == 0.0:
        assert (g_col == 0).all()  # the depth gradient alone
    else:
        assert _nrel(g_col, want_col) <= 1e-3
    assert (o["g_col"][:, 3:] == 0).all()
    # exact zeros: past the early stop, the overflow ray's rows
    a = int(c["offs"][c["stop_ray"]])
    for g in (g_col[a + 6:a + 96], g_h0[a + 6:a + 96], g_col[int(c["offs"][-1]):], g_h0[int(c["offs"][-1]):]):
        assert g.size and (g == 0).all()
    assert (g_h0[a:a + 5] != 0).all()  # (the stopping sample itself ends with T = 0: its density gradient is 0)
    # a ray whose target is masked out takes no depth gradient: with the colour
    # term off as well, its rows are exactly zero
    if cw == 0.0:
        for n in np.flatnonzero(c["masked"] & c["valid"]):
            assert (g_h0[c["offs"][n]:c["offs"][n] + COUNTS[n]] == 0).all(), n
    if live:
        # the live list: the rows with a nonzero gradient, in ray order (a row
        # live through the depth term alone is listed)
        nz = np.flatnonzero((g_col != 0).any(1) | (g_h0 != 0))
        total = int(o["total"][0])
        assert total == nz.size > 0
        assert np.array_equal(o["rows"].numpy()[:total], nz)


@pytest.mark.parametrize("live", [False, True])
def test_unit_weights_equal_the_colour_only_entries(cuda, loss_case, live):
    """(cw, dw) = (1, 0) through the depth entry: the colour-only entry's
    outputs bit for bit (and the _live form's lists)."""
    c = loss_case
    a = _run_loss(cuda, c, 1.0, 0.0, live=live)
    b = _run_loss(cuda, c, live=live)
    for name in ("loss", "g_col", "g_h"):
        va, vb = a[name], b[name]
        if name == "g_h":
            va, vb = va[:, 0], vb[:, 0]  # (the kernel writes column 0; 1..15 belong to the glue backward)
        assert torch.equal(va.contiguous().view(torch.int16 if va.dtype == torch.float16 else torch.int32),
                           vb.contiguous().view(torch.int16 if vb.dtype == torch.float16 else torch.int32)), name
    if live:
        total = int(b["total"][0])
        assert int(a["total"][0]) == total > 0
        assert torch.equal(a["rows"][:total], b["rows"][:total]) and torch.equal(a["cnt"], b["cnt"])


# ---- 3. the whole step against autograd ---------------------------------------------
def test_depth_step_matches_autograd(cuda, scenes):
    """FusedTrainer._forward_backward against Trainer._forward_backward (the
    reference's loss through the autograd ops) on the same batch, with
    test_fused_forward_backward_matches_autograd's bounds. RGB images: both
    blend on white, so the batch needs no shared random background."""
    from nerf.train import Trainer
    data = _dataset(scenes["rgb32"], cuda)
    f32 = _dataset(scenes["rgb32"], cuda, store="float32")
    assert data.images.shape == (6, 32, 32, 3) and data.depths.shape == (6, 32, 32)
    base = _model(cuda)
    ref, plain_model = copy.deepcopy(base), copy.deepcopy(base)
    ref.mean_count = 30000

    def fused(model, dw):
        ft = _trainer(cuda, data, model=model, depth_loss_weight=dw)
        ft._sample()
        ft.noises.zero_()  # the autograd step marches with perturb=False
        ft._forward_backward()
        torch.cuda.synchronize()
        return ft

    ft = fused(base, 0.5)
    gt = f32.images[int(ft.image_index)].view(-1, 3)[ft.pix.long()]
    in_mask = (ft.gt_depth >= 0.2) & (ft.gt_depth <= 1.0)
    assert N_RAYS // 50 < int(in_mask.sum()) < N_RAYS
    tr = Trainer(ref, data, depth_loss_weight=0.5, perturb=False, update_density=False)
    assert float(tr.scaler.get_scale()) == ft.scale
    batch = {"rays_o": ft.rays_o.clone()[None], "rays_d": ft.rays_d.clone()[None], "images": gt[None],
             "depths": ft.gt_depth.clone()[None]}
    ref.train()
    loss = tr._forward_backward(batch)
    torch.cuda.synchronize()
    assert int(ft.counter[0]) == int(ref.step_counter[0, 0]) > 0
    fused_loss = float(ft.loss_ray.double().sum()) / ft.N
    fused_dep = float(ft.loss_depth_ray.double().sum()) / ft.N
    lv, dv = float(loss.detach()), float(tr.last_depth_loss)
    print(f"samples {int(ft.counter[0])} loss fused {fused_loss:.8f} autograd {lv:.8f}; depth term {fused_dep:.8f} "
          f"/ {dv:.8f}")
    assert abs(fused_loss - lv) <= 1e-3 * abs(lv) + 1e-7
    assert dv > 0 and abs(fused_dep - dv) <= 1e-3 * dv + 1e-7
    refs = [ref.encoder.embeddings.grad, ref.sigma_net.weights.grad, ref.color_net.weights.grad]
    for name, g, r in zip(["embeddings", "sigma_net", "color_net"], ft.grads, refs):
        print(f"grad {name} rel {_rel(g, r):.3e}")
        assert torch.isfinite(g.float()).all(), name
        assert r.abs().max() > 0, name
        assert _rel(g, r) < 1e-2, (name, _rel(g, r))
    # ... and the depth term is in that gradient: the colour-only step's differs by more than the bound
    ft0 = fused(plain_model, 0.0)
    assert torch.equal(ft0.pix, ft.pix) and not ft0._depth
    away = _rel(ft0.grads[0], refs[0])
    print(f"colour-only embeddings grad rel {away:.3e}")
    assert away > 1e-2


# ---- 4. no change when off ----------------------------------------------------------
def test_zero_depth_weight_changes_nothing(cuda, scenes):
    """A dataset with depth maps and the default weights: the colour-only
    step's launches, so 20 steps (eager, then captured) end bit-identical to
    the same run on the dataset without depth maps."""
    with_d, without = _dataset(scenes["lego32"], cuda), _dataset(scenes["lego32_plain"], cuda)
    assert with_d.depths is not None and without.depths is None
    assert torch.equal(with_d.images, without.images) and torch.equal(with_d.poses, without.poses)
    a, b = _trainer(cuda, with_d, depth_loss_weight=0.0), _trainer(cuda, without)
    assert not a._depth and a._loss_job is None and not a._src.depths and a.last_depth_loss is None
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


# ---- 5. it learns -------------------------------------------------------------------
def test_depth_supervision_lowers_the_heldout_depth_error(cuda, scenes):
    """8 RGBA views at 64 x 64 and a 9th the training never saw, the seed and
    step count of test_training_on_images_learns_the_scene, on a scene where the
    target and the composite's depth mean the same thing. The composite measures
    from the march's start t0, not from the camera (the inherited offset,
    DESIGN.md section 12), so the poses are loaded at scale 0.6: the cameras
    (radius ~1.9) stand inside a bound-2 box, where t0 = min_near, and min_near
    is 0.02. The default depth_scale = scale puts the maps at 1.6-2.1, all but a
    few grazing hits inside the mask. The occupancy is a loose ball around the
    solid, as early in a real run: colour alone leaves density in front of the
    surfaces there, which is what the depth term is for."""
    from nerf.eval import depth_error, psnr
    from nerf.provider import sphere_bitfield
    s = 0.6
    data = _dataset(scenes["lego64"], cuda, scale=s, depth_scale=None)
    val = _dataset(scenes["lego64"], cuda, type="val", scale=s, depth_scale=None)
    assert data.depth_scale == s and data.depths.shape == (8, 64, 64) and val.depths.shape == (1, 64, 64)
    assert float(data.poses[:, :3, 3].abs().max()) < 2.0
    gt = val.depths[0] * s
    in_mask = (gt >= 0.02) & (gt <= 2.0)  # (a few grazing hits of the far box lie past the bound)
    assert int(in_mask.sum()) > 0.8 * int((gt > 0).sum()) > 64 * 64 // 50
    out = {}
    for dw in (0.0, 1.0):
        model = _model(cuda, bound=2, bits=sphere_bitfield(0.7 * s, cascade=2, bound=2.0), min_near=0.02)
        ft = _trainer(cuda, data, model=model, M=2 * M_ROWS, depth_loss_weight=dw)
        for _ in range(4):
            ft.step()
        ft.capture()
        ft.run(200)
        ft.flush()
        torch.cuda.synchronize()
        assert ft.device_errors() == 0 and np.isfinite(ft.last_loss) and ft.sample_count() < ft.M
        out[dw] = (depth_error(ft.model, val, 0), psnr(ft.model, val, 0), ft.last_loss, ft.last_depth_loss)
        print(f"depth_loss_weight {dw}: held-out depth error {out[dw][0]:.6f}, PSNR {out[dw][1]:.4f}, "
              f"loss {out[dw][2]:.6f}, depth term {out[dw][3]}")
    assert np.isfinite(out[0.0][0]) and np.isfinite(out[1.0][0])
    assert out[1.0][0] < out[0.0][0]
    assert np.isfinite(out[1.0][1]) and np.isfinite(out[0.0][1])


# ---- 6. main_nerf -------------------------------------------------------------------
def test_main_nerf_trains_with_depth_and_reports_it(cuda, scenes, tmp_path, capsys):
    import main_nerf
    args = ["-O", "--workspace", str(tmp_path / "ws"), "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--iters",
            "64", "--num_rays", "1024", "--sample_budget", "131072", "--depth_loss_weight", "0.5"]
    out = main_nerf.main([scenes["lego64"], *args, "--depth_scale", str(DEPTH_SCALE)])
    text = capsys.readouterr().out
    assert "PSNR" in text and "depth error" in text and "(rgb " in text and ", dep " in text
    assert np.isfinite(out["psnr"]) and np.isfinite(out["loss"])
    assert out["depth_error"] is not None and np.isfinite(out["depth_error"]) and out["depth_error"] > 0
    # a scene without dep_path: the trainer's ValueError text, as the exit message
    with pytest.raises(SystemExit) as e:
        main_nerf.main([scenes["lego32_plain"], *args])
    assert "depth_loss_weight" in str(e.value.code) and "depth maps" in str(e.value.code)
