"""Error-map importance sampling on the fused engine:
the device's weighted draw without replacement (ngp_error_map_select), the
draw's cell -> pixel rule at all three image draw sites, the map's EMA update
and the plumbing up to main_nerf.py --error_map, against the numpy restatement
in tests/error_map_helpers.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import error_map_helpers as eh
from depth_helpers import write_scene

pytestmark = pytest.mark.gpu

M_ROWS = 30080  # a multiple of 128
DRAW = 9        # StepState.draw, as an int32 index into the state


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    def make(name, *args, **kw):
        return write_scene(str(tmp_path_factory.mktemp(name)), *args, **kw)
    return {"odd": make("odd", 3, 20, 28, colmap=True, depth=False, num_rays=32),
            "lego32": make("lego32", 6, 32, 32, depth=True, num_rays=128),
            "lego64": make("lego64", 8, 64, 64, depth=False, heldout=1, num_rays=128)}


def _dataset(path, dev, num_rays, res=None, store="uint8", type="train", fill=None):
    """A dataset with a res x res map (res None: no map); fill: a seed for a
    random positive map in place of the ones. (depth_scale 0.25: the depth maps'
    distances of 2..4 inside the bound-1 model's [min_near, bound].)"""
    from nerf.provider import NeRFDataset
    data = NeRFDataset(path, dev, type=type, scale=1.0, num_rays=num_rays, store=store, error_map=res is not None,
                       error_map_res=res or 128, depth_scale=0.25)
    if fill is not None:
        g = torch.Generator().manual_seed(fill)
        data.error_map.copy_(torch.rand(data.error_map.shape, generator=g) + 0.05)
    return data


def _model(dev):
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    with torch.no_grad():
        model.encoder.embeddings.normal_(0, 0.05)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(dev))
    return model


def _trainer(dev, data, seed=3, options=None, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(_model(dev), data, M=M_ROWS, seed=seed, options=options, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the select kernel on its own ------------------------------------------------
class Select:
    """ngp_error_map_select on its own state and buffers."""

    def __init__(self, dev, n_poses, res, seed):
        import _ngp_native as nat
        self.nat, self.lib, self.dev = nat, nat.lib(), dev
        self.n_poses, self.res, self.seed = n_poses, res, seed
        self.state = torch.zeros(self.lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=dev)
        nat.check(self.lib.ngp_fused_state_init(nat.ptr(self.state), 65536.0, nat.stream_of(self.state)), "init")
        self.keys = torch.zeros(res * res, device=dev)

    def __call__(self, w, N, it, out=None, keys=True):
        nat = self.nat
        self.state.view(torch.int32)[DRAW] = it
        sel = torch.full((N,), -1, dtype=torch.int32, device=self.dev) if out is None else out
        nat.check(self.lib.ngp_error_map_select(nat.ptr(w), self.n_poses, self.res, N, self.seed,
                                                nat.ptr(self.state), nat.ptr(sel),
                                                nat.ptr(self.keys) if keys else None, nat.stream_of(w)), "select")
        return sel


@pytest.mark.parametrize("res,N", [(4, 5), (16, 64), (128, 4096), (128, 16384)])
def test_select_is_the_top_n_of_the_race(cuda, res, N):
    """Keys against the float64 oracle to 1e-5 relative (one logf and one divide
    are a few fp32 ulp, ~4e-7: more than 10x margin); the selection exactly the
    top N of the device's own keys under the tie rule, ascending, and the same
    bytes on a second run."""
    seed, it, n_poses = 11, 5, 3
    C = res * res
    g = torch.Generator().manual_seed(res * 100003 + N)
    w = (torch.rand(n_poses, C, generator=g) + 0.05).to(cuda)
    run = Select(cuda, n_poses, res, seed)
    sel = run(w, N, it)
    keys = run.keys.clone()
    sel2 = run(w, N, it)
    torch.cuda.synchronize()
    assert torch.equal(sel, sel2) and torch.equal(_bits(keys), _bits(run.keys))
    pose = eh.pose_of(seed, it, n_poses)
    want = eh.keys64(w[pose].cpu().numpy(), seed, it)
    got = keys.cpu().numpy()
    rel = np.abs(got.astype(np.float64) - want) / want
    print(f"res {res} N {N}: pose {pose}, keys max rel err {rel.max():.3e}")
    assert np.isfinite(got).all() and (got > 0).all()
    assert rel.max() <= 1e-5
    s = sel.cpu().numpy().astype(np.int64)
    assert (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < C
    assert np.array_equal(s, eh.top_n(got, N))
    assert int(run.state.view(torch.int32)[DRAW]) == it  # the select draws nothing itself


def test_select_edge_weights(cuda):
    res, N, n_poses, seed = 16, 64, 4, 21
    C = res * res
    run = Select(cuda, n_poses, res, seed)
    g = torch.Generator().manual_seed(7)
    for it in range(6):
        pose = eh.pose_of(seed, it, n_poses)
        # exactly N positive cells in the row that is read; the other rows would select differently
        pos = torch.randperm(C, generator=g)[:N]
        w = torch.zeros(n_poses, C)
        w[:, [c for c in range(C) if c not in set(pos.tolist())][:N]] = 1.0
        w[pose] = 0.0
        w[pose, pos] = torch.rand(N, generator=g) + 1e-3
        sel = run(w.to(cuda), N, it)
        assert sel.tolist() == sorted(pos.tolist()), (it, pose)
        # all-zero weights: cells 0 .. N - 1 (every key ties at 0)
        sel = run(torch.zeros(n_poses, C, device=cuda), N, it)
        assert sel.tolist() == list(range(N)), it
        assert int(run.keys.abs().sum()) == 0
        # one cell 1e30 times heavier than the rest is always in
        heavy = int(torch.randint(0, C, (1,), generator=g))
        w = torch.full((n_poses, C), 1e-20)
        w[pose, heavy] = 1e10
        sel = run(w.to(cuda), N, it)
        assert heavy in sel.tolist(), (it, heavy)
    # negative and NaN weights count as zero
    w = torch.ones(n_poses, C)
    w[:, :C - N] = torch.tensor([-1.0, float("nan")]).repeat((C - N) // 2)
    sel = run(w.to(cuda), N, 0)
    assert sel.tolist() == list(range(C - N, C))
    # without the keys buffer: the same selection
    assert torch.equal(run(w.to(cuda), N, 0, keys=False), sel)


def test_select_uniform_weights_include_every_cell_equally_often(cuda):
    """200 draws of 64 of 256 equal cells: every cell's inclusion count within
    5 binomial standard deviations of 200 * 64 / 256 = 50 (sigma = sqrt(200 * 0.25 * 0.75)
    = 6.1). The seed is the first at which the CPU oracle itself passes."""
    res, N, draws = 16, 64, 200
    C, p = res * res, N / (res * res)
    lo, hi = draws * p - 5 * math.sqrt(draws * p * (1 - p)), draws * p + 5 * math.sqrt(draws * p * (1 - p))
    for seed in range(1, 20):
        ref = eh.inclusion_counts(res, N, draws, seed)
        if lo <= ref.min() and ref.max() <= hi:
            break
    else:
        pytest.fail("no seed at which the oracle passes")
    run = Select(cuda, 1, res, seed)
    w = torch.ones(1, C, device=cuda)
    sel = torch.zeros(draws, N, dtype=torch.int32, device=cuda)
    for it in range(draws):
        run(w, N, it, out=sel[it], keys=False)
    counts = np.bincount(sel.cpu().numpy().ravel(), minlength=C)
    print(f"seed {seed}: counts {counts.min()}..{counts.max()} (oracle {ref.min()}..{ref.max()}), bounds "
          f"{lo:.1f}..{hi:.1f}")
    assert counts.sum() == draws * N and counts.size == C
    assert lo <= counts.min() and counts.max() <= hi


def test_select_argument_errors(cuda):
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    w = torch.ones(2, 16, device=cuda)
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    sel = torch.full((16,), -7, dtype=torch.int32, device=cuda)
    s = nat.stream_of(w)
    ERR_ARG = -1  # NGP_ERR_ARG
    bad = [(None, 2, 4, 4, P(state), P(sel)), (P(w), 2, 0, 1, P(state), P(sel)), (P(w), 2, 129, 4, P(state), P(sel)),
           (P(w), 2, 4, 0, P(state), P(sel)), (P(w), 2, 4, 17, P(state), P(sel)), (P(w), 0, 4, 4, P(state), P(sel)),
           (P(w), 2, 4, 4, None, P(sel)), (P(w), 2, 4, 4, P(state), None)]
    for m, n_poses, res, N, st, out in bad:
        assert lib.ngp_error_map_select(m, n_poses, res, N, 0, st, out, None, s) == ERR_ARG, (n_poses, res, N)
        assert lib.ngp_last_error()
    torch.cuda.synchronize()
    assert bool((sel == -7).all()) and bool((w == 1).all())
    # ... and the update entry's
    z = torch.zeros(16, 4, device=cuda)
    zi = torch.zeros(16, 3, dtype=torch.int32, device=cuda)
    ok = [P(w), 2, 4, 16, P(zi), P(z), P(z), 4, P(z), P(zi), P(zi)]
    for k, v in ((0, None), (4, None), (5, None), (6, None), (8, None), (9, None), (10, None), (1, 0), (2, 0), (2, 129),
                 (3, 17), (7, 5)):
        args = list(ok)
        args[k] = v
        assert lib.ngp_error_map_update(*args, s) == ERR_ARG, (k, v)
    torch.cuda.synchronize()
    assert bool((w == 1).all())


def _image_entries(lib, nat, src, N, state, dev):
    """The three image draw entries on an ngp_image_source, as return codes."""
    P = nat.ptr
    f = torch.zeros(N, 4, device=dev)
    poses = torch.eye(4, device=dev)[None].contiguous()
    intr = (ctypes.c_float * 4)(30.0, 30.0, 4.0, 4.0)
    aabb = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    s = nat.stream_of(f)
    bufs = [P(f)] * 7
    rays = lib.ngp_image_rays(P(poses), 1, intr, 8, 8, N, ctypes.byref(src), aabb, 0.2, 0, P(state), *bufs, P(cnt),
                              None, s)
    head = lib.ngp_fused_step_head_images(P(poses), 1, intr, 8, 8, N, ctypes.byref(src), aabb, 0.2, 0, P(state),
                                          *bufs, P(cnt), None, 2.0, 0.5, 2000, 1, P(f), 0, None, None, None, None,
                                          None, None, 0, s)
    bj = nat.BatchJob()
    bj.poses, bj.n_poses, bj.intrinsics4, bj.H, bj.W, bj.N = P(poses), 1, ctypes.addressof(intr), 8, 8, N
    bj.aabb6, bj.state, bj.counter = ctypes.addressof(aabb), P(state), P(cnt)
    grid = lib.ngp_grid_encode_backward_fused_reduce_batch_images(
        None, None, 1.0, None, None, 0, None, None, 3, 2, 16, 0.5, 16, 0, 0, 0, None, None, 0, 0, None, 2, None, None,
        None, None, None, None, None, ctypes.byref(bj), ctypes.byref(src), s)
    return rays, head, grid


def test_image_source_rejects_inconsistent_map_fields(cuda):
    """Every inconsistent combination of the map fields is NGP_ERR_ARG at all
    three draw sites, before any device work (the buffers keep their fill)."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    N = 16
    pixels = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=cuda)
    emap = torch.ones(1, 16, device=cuda)
    sel = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    coarse = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)

    def source(**kw):
        src = nat.ImageSource()
        src.pixels, src.channels, src.dtype = P(pixels), 4, nat.DTYPE_U8
        src.error_map, src.error_map_res, src.selected, src.perm_mult, src.coarse = P(emap), 4, P(sel), 7, P(coarse)
        for k, v in kw.items():
            setattr(src, k, v)
        return src

    cases = [dict(error_map_res=0), dict(error_map_res=129), dict(selected=None), dict(coarse=None),
             dict(error_map_res=3),   # N = 16 > 9 cells
             dict(perm_mult=0), dict(perm_mult=4), dict(perm_mult=17),  # not a permutation of 16
             dict(error_map=None), dict(error_map=None, selected=None, coarse=None, perm_mult=0),  # res without a map
             dict(error_map=None, error_map_res=0, selected=None, coarse=None)]  # perm_mult without a map
    for kw in cases:
        codes = _image_entries(lib, nat, source(**kw), N, state, cuda)
        assert codes == (-1, -1, -1), (kw, codes)  # NGP_ERR_ARG
    torch.cuda.synchronize()
    assert bool((sel == -7).all()) and bool((coarse == -7).all()) and bool((emap == 1).all())
    assert int(state.view(torch.int32)[DRAW]) == 0


# ---- the draw ----------------------------------------------------------------------
def test_draw_takes_its_pixels_from_the_selected_cells(cuda, scenes):
    """H = 20, W = 28, res 8 (neither a multiple), N = 32, through _sample():
    coarse is the permutation of `selected`, pix the cell -> pixel rule, the
    target that pixel; the streams that do not depend on the pixel are a
    map-less trainer's. ngp_image_rays after a select of its own draws the same."""
    import raymarching

    import _ngp_native as nat
    from nerf.utils import get_rays
    H, W, res, N, seed = 20, 28, 8, 32, 3
    data = _dataset(scenes["odd"], cuda, N, res=res, fill=1)
    f32 = _dataset(scenes["odd"], cuda, N, store="float32")
    assert (data.H, data.W) == (H, W) and data.error_map.shape == (3, res * res)
    a, b = _trainer(cuda, data, seed=seed), _trainer(cuda, data, seed=seed, error_map=False)
    assert a._emap is data.error_map and b._emap is None and a._src.perm_mult == eh.perm_mult(N) == 19
    emap0 = data.error_map.clone()
    for it in range(3):
        a._sample()
        b._sample()
        torch.cuda.synchronize()
        pose = eh.pose_of(seed, it, 3)
        assert int(a.image_index) == int(b.image_index) == pose
        sel = a.selected.cpu().numpy()
        # (the selection itself: the top N of the oracle's keys; fp32 / fp64 keys order alike here)
        assert np.array_equal(sel, eh.top_n(eh.keys64(emap0[pose].cpu().numpy(), seed, it), N)), it
        coarse = eh.coarse_of(sel, seed, it)
        assert np.array_equal(a.coarse.cpu().numpy(), coarse), it
        assert sorted(coarse.tolist()) == sel.tolist()
        pix = eh.pix_of(coarse, H, W, res, seed, it)
        assert np.array_equal(a.pix.cpu().numpy(), pix), it
        want = f32.images[pose].view(-1, 4)[a.pix.long()]
        assert torch.equal(_bits(a.rgba), _bits(want)), it
        for name in ("rays_o", "bg", "noises"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (it, name)
        assert not torch.equal(a.pix, b.pix)
        rays = get_rays(data.poses[pose:pose + 1], data.intrinsics, H, W, -1)
        assert torch.allclose(a.rays_d, rays["rays_d"][0][a.pix.long()], atol=1e-6)
        nears, fars = raymarching.near_far_from_aabb(a.rays_o, a.rays_d, a.model.aabb_train, a.model.min_near)
        assert torch.equal(_bits(nears), _bits(a.nears)) and torch.equal(_bits(fars), _bits(a.fars))
    assert torch.equal(_bits(data.error_map), _bits(emap0))  # a draw alone leaves the map alone
    # the third draw site, ngp_image_rays, on its own state at draw 2
    lib, P = nat.lib(), nat.ptr
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), 65536.0, s), "fused_state_init")
    state.view(torch.int32)[DRAW] = 2
    f = {k: torch.zeros(N, w, device=cuda) for k, w in (("rays_o", 3), ("rays_d", 3), ("rgba", 4), ("bg", 3))}
    f.update({k: torch.zeros(N, device=cuda) for k in ("nears", "fars", "noises")})
    i32 = dict(dtype=torch.int32, device=cuda)
    pix, index, sel, coarse = (torch.full((n,), -1, **i32) for n in (N, 1, N, N))
    counter = torch.zeros(2, **i32)
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = P(data.images), 4, nat.DTYPE_U8
    src.pix, src.image_index = P(pix), P(index)
    src.error_map, src.error_map_res, src.selected, src.coarse = P(data.error_map), res, P(sel), P(coarse)
    src.perm_mult = eh.perm_mult(N)
    nat.check(lib.ngp_error_map_select(P(data.error_map), 3, res, N, seed, P(state), P(sel), None, s), "select")
    nat.check(lib.ngp_image_rays(P(data.poses), 3, a._intr, H, W, N, ctypes.byref(src), a._aabb,
                                 float(a.model.min_near), seed, P(state), P(f["rays_o"]), P(f["rays_d"]),
                                 P(f["rgba"]), P(f["bg"]), P(f["nears"]), P(f["fars"]), P(f["noises"]), P(counter),
                                 None, s), "image_rays")
    torch.cuda.synchronize()
    for name, t in f.items():
        assert torch.equal(_bits(t), _bits(getattr(a, name))), name
    assert torch.equal(pix, a.pix) and torch.equal(index, a.image_index)
    assert torch.equal(sel, a.selected) and torch.equal(coarse, a.coarse)
    assert int(state.view(torch.int32)[DRAW]) == 3


@pytest.mark.parametrize("live", [True, False])
def test_draw_sites_draw_the_same_batches_with_the_map_on(cuda, scenes, live):
    """The draw in the grid backward's bin launch (draw_ahead) against the draw
    in the head launch, both from the map as the steps before left it: the same
    batches, losses and map bytes (after step i, a holds batch i + 1)."""
    N, res = 128, 16
    da, db = (_dataset(scenes["lego32"], cuda, N, res=res, fill=2) for _ in range(2))
    a = _trainer(cuda, da, options=dict(live_rows=live))
    b = _trainer(cuda, db, options=dict(live_rows=live, draw_ahead=False))
    assert a._draw_ahead and a._live == live and not b._draw_ahead and a._emap is da.error_map
    batches = []
    for i in range(4):
        if i < 3:
            a.step()
        b.step()
        torch.cuda.synchronize()
        if i > 0:
            pa, ca, ra, ia = batches[i - 1]
            assert torch.equal(pa, b.pix) and torch.equal(ca, b.coarse) and torch.equal(ia, b.image_index), i
            assert torch.equal(_bits(ra), _bits(b.rgba)), i
        if i < 3:
            assert a._ahead
            batches.append((a.pix.clone(), a.coarse.clone(), a.rgba.clone(), a.image_index.clone()))
            assert a.sample_count() == b.sample_count() > 0, i
            assert a.last_loss == b.last_loss and np.isfinite(a.last_loss), i
            assert torch.equal(_bits(da.error_map), _bits(db.error_map)), i
    assert not torch.equal(da.error_map, torch.ones_like(da.error_map))


def test_a_trainer_without_the_map_draws_what_it_drew_before(cuda, scenes):
    """error_map=False on a dataset that has a map: the uniform draw of a
    dataset without one, bit for bit, step after step, and the map untouched."""
    N = 128
    plain, mapped = _dataset(scenes["lego32"], cuda, N), _dataset(scenes["lego32"], cuda, N, res=16)
    a, b = _trainer(cuda, plain), _trainer(cuda, mapped, error_map=False)
    assert a._emap is None and b._emap is None and not hasattr(b, "coarse")
    assert b._src.error_map is None and b._src.selected is None and b._src.perm_mult == 0
    for i in range(3):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert torch.equal(a.pix, b.pix) and torch.equal(a.image_index, b.image_index), i
        for name in ("rays_o", "rays_d", "rgba", "bg", "noises", "nears", "fars", "loss_ray"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (i, name)
        assert a.last_loss == b.last_loss
    a.flush()
    b.flush()
    for p, q in zip(a.params, b.params):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))
    assert bool((mapped.error_map == 1).all())
    assert "error_map" not in b.checkpoint(full=False)


# ---- the EMA update ----------------------------------------------------------------
def _check_ema(ft, data, before):
    """The map after one step of a draw_ahead=False trainer (its buffers still
    hold the step's batch) -> the step's per-ray colour errors by ray row."""
    torch.cuda.synchronize()
    N = ft.N
    pose = int(ft.image_index)
    index = ft.rays[:, 0].long().cpu().numpy()
    assert sorted(index.tolist()) == list(range(N))
    cells = ft.coarse.cpu().numpy().astype(np.int64)[index]
    assert np.unique(cells).size == N
    err = eh.colour_err(ft.out_image.cpu().numpy()[index], ft.rgba.cpu().numpy()[index], ft.bg.cpu().numpy()[index])
    want = before.cpu().numpy().copy()
    want[pose, cells] = eh.ema(want[pose, cells], err)
    got = data.error_map.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[pose, cells] != before.cpu().numpy()[pose, cells]).any()
    return err


def test_ema_folds_the_rays_colour_loss_into_their_cells(cuda, scenes):
    """One step from a random positive map: the drawn image's row at the batch's
    cells is 0.1f * old + 0.9f * err, err the engine's own per-ray loss through
    rays[:, 0]; every other cell and row keeps its bits. Rays without samples
    are updated too."""
    N = 128
    data = _dataset(scenes["lego32"], cuda, N, res=16, fill=4)
    before = data.error_map.clone()
    ft = _trainer(cuda, data, options=dict(draw_ahead=False))
    ft.step()
    err = _check_ema(ft, data, before)
    assert np.array_equal(err.view(np.uint32), ft.loss_ray.cpu().numpy().view(np.uint32))
    assert int((ft.rays[:, 2] == 0).sum()) > 0 and int((ft.rays[:, 2] > 0).sum()) > 0
    assert err.min() >= 0 and err.max() > 0


def test_ema_uses_the_colour_term_alone_under_depth_supervision(cuda, scenes):
    N = 128
    data = _dataset(scenes["lego32"], cuda, N, res=16, fill=5)
    assert data.depths is not None
    before = data.error_map.clone()
    ft = _trainer(cuda, data, options=dict(draw_ahead=False), depth_loss_weight=0.5, color_loss_weight=0.7)
    ft.step()
    err = _check_ema(ft, data, before)
    total = ft.loss_ray.cpu().numpy()
    assert float(ft.loss_depth_ray.sum()) > 0  # the depth term is in the loss, and not in the map
    assert not np.array_equal(err.view(np.uint32), total.view(np.uint32))
    np.testing.assert_allclose(0.7 * err + 0.5 * ft.loss_depth_ray.cpu().numpy(), total, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("what", ["table", "color_net"])
def test_a_non_finite_field_leaves_the_map_finite(cuda, scenes, what):
    """The table set to inf (the networks' ReLUs may still give finite colours),
    and the colour network's weights set to NaN (they cannot): the map stays
    finite and >= 0, and a ray with a non-finite error keeps its cell's bits."""
    N = 128
    data = _dataset(scenes["lego32"], cuda, N, res=16, fill=6)
    before = data.error_map.clone()
    ft = _trainer(cuda, data, options=dict(draw_ahead=False))
    with torch.no_grad():
        if what == "table":
            ft.params[0].fill_(float("inf"))
        else:
            ft.params[2].fill_(float("nan"))
    ft.sync_half()
    ft.step()
    torch.cuda.synchronize()
    m = data.error_map
    assert bool(torch.isfinite(m).all()) and bool((m >= 0).all())
    hit = ft.rays[:, 2] > 0
    assert int(hit.sum()) > 0
    bad = ~torch.isfinite(ft.out_image).all(-1)  # by ray index
    print(f"{what}: {int(hit.sum())} rays with samples, {int(bad.sum())} non-finite colours")
    if what == "color_net":
        assert bool(bad[ft.rays[hit, 0].long()].all())
    pose = int(ft.image_index)
    cells = ft.coarse[bad].long()
    assert torch.equal(_bits(m[pose, cells]), _bits(before[pose, cells]))
    good = ft.coarse[~bad].long()
    assert not torch.equal(_bits(m[pose, good]), _bits(before[pose, good]))


# ---- graphs, checkpoints, arguments ------------------------------------------------
def test_graph_replays_equal_eager_steps(cuda, scenes):
    """capture() + run(k) with the map on: the map bytes and the parameters of
    k eager step() calls from the same state (the density update in between too)."""
    N = 128
    da, db = (_dataset(scenes["lego32"], cuda, N, res=16, fill=8) for _ in range(2))
    a, b = _trainer(cuda, da), _trainer(cuda, db)
    for _ in range(3):
        a.step()
        b.step()
    a.capture(warmup=0, multi=3)
    a.run(7)
    assert a.eager_steps == 3
    for _ in range(7):
        b.step()
    a.update_density()
    b.update_density()
    a.run(2)
    b.step()
    b.step()
    a.flush()
    b.flush()
    torch.cuda.synchronize()
    assert torch.equal(_bits(da.error_map), _bits(db.error_map))
    assert not bool((da.error_map == 1).all()) and bool(torch.isfinite(da.error_map).all())
    for p, q in zip(a.params, b.params):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))
    assert a.last_loss == b.last_loss and np.isfinite(a.last_loss)
    assert a.device_errors() == 0


def test_checkpoint_round_trip_restores_the_map(cuda, scenes):
    N = 128
    da, db = (_dataset(scenes["lego32"], cuda, N, res=16) for _ in range(2))
    a, b = _trainer(cuda, da), _trainer(cuda, db)
    for _ in range(3):
        a.step()
    state = a.checkpoint()
    assert state["error_map"].shape == (6, 256) and state["error_map"].device.type == "cpu"
    assert not bool((state["error_map"] == 1).all())
    b.load_checkpoint(state)
    assert torch.equal(_bits(db.error_map), _bits(da.error_map))
    # ... and the restored trainer goes on as the saved one does
    a.step()
    b.step()
    a.flush()
    b.flush()
    torch.cuda.synchronize()
    assert torch.equal(_bits(db.error_map), _bits(da.error_map)) and a.last_loss == b.last_loss
    off = _trainer(cuda, _dataset(scenes["lego32"], cuda, N))
    off.step()
    assert "error_map" not in off.checkpoint()
    off.load_checkpoint(state)  # a map in the checkpoint, none in the trainer: ignored


def test_trainer_argument_errors(cuda, scenes):
    """Every ValueError of FusedTrainer's error-map mode names its cause and is
    raised before any device work: the map keeps its bytes."""
    from nerf.provider import SyntheticLego
    N = 128
    data = _dataset(scenes["lego32"], cuda, N, res=16, fill=9)
    before = data.error_map.clone()
    with pytest.raises(ValueError, match="error map"):
        _trainer(cuda, _dataset(scenes["lego32"], cuda, N), error_map=True)
    with pytest.raises(ValueError, match="image dataset"):
        lego = SyntheticLego(cuda, H=32, W=32, n_poses=6, num_rays=N)
        lego.error_map, lego.error_map_res = torch.ones(6, 256, device=cuda), 16
        _trainer(cuda, lego, error_map=True)
    with pytest.raises(ValueError, match="num_rays"):
        _trainer(cuda, _dataset(scenes["lego32"], cuda, N, res=11))  # 121 cells < 128 rays
    with pytest.raises(ValueError, match="march_adam"):
        _trainer(cuda, data, options=dict(march_adam=False))
    good = data.error_map
    for bad, what in ((good[:, :255], "256"), (good.double(), "float32"), (good.cpu(), "cpu"),
                      (good.t().contiguous().t(), "contiguous"), (good[:5], "256")):
        data.error_map = bad
        with pytest.raises(ValueError, match=what):
            _trainer(cuda, data)
    data.error_map = good
    data.error_map_res = 200
    with pytest.raises(ValueError, match="error_map_res"):
        _trainer(cuda, data)
    data.error_map_res = 16
    torch.cuda.synchronize()
    assert torch.equal(_bits(good), _bits(before))
    assert _trainer(cuda, data)._emap is good  # ... and the repaired dataset is accepted


def test_world_size_above_one_is_rejected(cuda, scenes, monkeypatch):
    import torch.distributed as dist
    data = _dataset(scenes["lego32"], cuda, 128, res=16)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 0)
    with pytest.raises(ValueError, match="world size"):
        _trainer(cuda, data, distributed=True)
    assert bool((data.error_map == 1).all())


# ---- behaviour ---------------------------------------------------------------------
def test_the_map_steers_the_rays_onto_the_object(cuda, scenes):
    """64 x 64 Lego views (alpha > 0 on under a fifth of the pixels), res 16,
    N = 128, 300 steps, same seed: over the last 50 draws the share of rays on
    alpha > 0 pixels with the map on exceeds the uniform sampler's by more than
    3 binomial standard deviations of the uniform share over those 50 * 128 rays."""
    N, steps, last = 128, 300, 50
    on, off = _dataset(scenes["lego64"], cuda, N, res=16), _dataset(scenes["lego64"], cuda, N)
    alpha = (on.images[..., 3] > 0)
    cover = float(alpha.float().mean())
    assert cover < 0.2
    a, b = _trainer(cuda, on), _trainer(cuda, off)
    hits = {"on": 0, "off": 0}
    for i in range(steps):
        a.step()
        b.step()
        if i >= steps - last:
            for name, ft in (("on", a), ("off", b)):
                hits[name] += int(alpha[int(ft.image_index)].view(-1)[ft.pix.long()].sum())
    total = last * N
    p_on, p_off = hits["on"] / total, hits["off"] / total
    sigma = math.sqrt(p_off * (1 - p_off) / total)
    print(f"coverage {cover:.4f}; share on the object: map on {p_on:.4f}, off {p_off:.4f} (sigma {sigma:.4f}); "
          f"loss on {a.last_loss:.6f} off {b.last_loss:.6f}")
    assert p_on > p_off + 3 * sigma
    assert a.device_errors() == 0 and np.isfinite(a.last_loss)


def test_main_nerf_error_map(cuda, scenes, tmp_path, capsys):
    import main_nerf
    ws = str(tmp_path / "ws")
    out = main_nerf.main([scenes["lego64"], "-O", "--workspace", ws, "--bound", "1", "--scale", "1.0", "--dt_gamma",
                          "0", "--iters", "64", "--num_rays", "128", "--sample_budget", "32768", "--error_map",
                          "--error_map_res", "16"])
    text = capsys.readouterr().out
    assert "PSNR" in text and "error map 16x16" in text
    assert np.isfinite(out["psnr"]) and np.isfinite(out["loss"])
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert state["global_step"] == 64
    m = state["error_map"]
    assert m.shape == (8, 256) and bool(torch.isfinite(m).all()) and bool((m >= 0).all()) and not bool((m == 1).all())
    with pytest.raises(SystemExit, match="num_rays"):
        main_nerf.main([scenes["lego64"], "-O", "--workspace", ws, "--bound", "1", "--scale", "1.0", "--iters", "1",
                        "--num_rays", "512", "--error_map", "--error_map_res", "16"])
    with pytest.raises(SystemExit, match="error_map_res"):
        main_nerf.main([scenes["lego64"], "-O", "--workspace", ws, "--error_map", "--error_map_res", "300"])


def test_reference_api_trainer_updates_the_map(cuda, scenes):
    """nerf.train.Trainer on a dataset with a map: batches from get_rays'
    error_map branch, each ray's colour MSE folded into its cell."""
    from nerf.train import Trainer
    data = _dataset(scenes["lego32"], cuda, 128, res=16, store="float32")
    model = _model(cuda)
    tr = Trainer(model, data, update_density=False)
    for _ in range(2):
        tr.train_step()
    torch.cuda.synchronize()
    m = data.error_map
    changed = (m != 1).sum(1)
    assert 128 <= int(changed.sum()) <= 256 and int((changed > 0).sum()) <= 2
    assert bool(torch.isfinite(m).all()) and bool((m >= 0).all())
