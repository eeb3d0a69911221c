"""GPU: csrc/dnerf.hip and the dnerf package on an MI355X: the (x, t)
encoding against float64, the time-sliced grid's query points, the EMA / global
mean / pack, update_extra_state against a torch restatement, the network
against its composition, training on a small moving scene, and the front door."""
import os

import numpy as np
import pytest
import torch

import dnerf_helpers as dh

pytestmark = pytest.mark.gpu

ARG_ERROR = -1


# ---- encode ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_encode_against_float64(cuda, N, parity_report):
    """Float and half output, contiguous rows and a wider row stride. Bound: 4 x the largest error of the
    repository's plain-torch float32 encoders against float64 on the same inputs (+ half a float16 ulp of the
    value for half output)."""
    import dnerf
    x, t = dh.encode_inputs(N, cuda)
    ref = dh.encode_ref(x.cpu().numpy(), t.cpu().numpy())
    torch_err = float(np.abs(dh.torch_encode(x, t).double().cpu().numpy() - ref).max())
    bound = 4 * torch_err
    out = dnerf.encode(x, t)
    err = float(np.abs(out.double().cpu().numpy() - ref).max())
    print(f"dnerf encode N={N}: torch fp32 err {torch_err:.3e} bound {bound:.3e} kernel err {err:.3e}")
    parity_report(f"N={N} torch fp32 err {torch_err:.3e} kernel err {err:.3e}")
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, 76)
    assert torch_err > 0 and err <= bound
    # the columns are the repository's frequency encoders' (the fast-sine kernels: |error| ~ |argument| 2^-23)
    from encoding import get_encoder
    fx, ft = get_encoder("frequency", multires=10)[0], get_encoder("frequency", input_dim=1, multires=6)[0]
    assert (torch.cat([fx(x), ft(t)], 1) - out).abs().max().item() < 1e-3
    # half output
    outh = dnerf.encode(x, t, torch.float16)
    errh = np.abs(outh.double().cpu().numpy() - ref)
    print(f"dnerf encode N={N}: half err {errh.max():.3e}")
    assert outh.dtype == torch.float16 and (errh <= bound + 0.5 * dh.half_ulp(ref)).all()
    # a wider row stride: the same bits, the columns past the row untouched
    for dtype, dense in ((torch.float32, out), (torch.float16, outh)):
        wide = torch.full((N, 83), 7.0, dtype=dtype, device=cuda)
        assert dnerf.encode(x, t, out=wide) is wide
        assert torch.equal(wide[:, :76], dense) and (wide[:, 76:] == 7.0).all()


@pytest.mark.parametrize("N", [1, 65])
def test_encode_one_time_for_all_rows(cuda, N):
    """Stride-0 t and a stride-1 t filled with the same value give equal bits."""
    import dnerf
    x, _ = dh.encode_inputs(N, cuda)
    t1 = torch.full((1, 1), 0.37, device=cuda)
    tN = torch.full((N, 1), 0.37, device=cuda)
    for dtype in (torch.float32, torch.float16):
        assert torch.equal(dnerf.encode(x, t1, dtype), dnerf.encode(x, tN, dtype))
    assert dnerf.encode(x[:0], t1).shape == (0, 76)


def test_encode_argument_errors(cuda):
    import _ngp_native as nat
    import dnerf
    x = torch.zeros(4, 3, device=cuda)
    with pytest.raises(RuntimeError):
        dnerf.encode(x, torch.zeros(3, 1, device=cuda))
    with pytest.raises(RuntimeError):
        dnerf.encode(x, torch.zeros(1, 1, device=cuda), out=torch.zeros(4, 75, device=cuda))
    out = torch.zeros(4, 76, device=cuda)
    lib = nat.lib()
    assert lib.ngp_dnerf_encode(x.data_ptr(), x.data_ptr(), 2, 4, out.data_ptr(), 0, 76, None) == ARG_ERROR
    assert lib.ngp_dnerf_encode(x.data_ptr(), x.data_ptr(), 0, 4, out.data_ptr(), 2, 76, None) == ARG_ERROR
    assert lib.ngp_dnerf_encode(x.data_ptr(), x.data_ptr(), 0, 4, out.data_ptr(), 0, 75, None) == ARG_ERROR
    assert lib.ngp_dnerf_encode(None, None, 0, 0, None, 0, 76, None) == 0


# ---- query points ----------------------------------------------------------------------
def _check_points(xyzs, times, indices, T, C, H, bound):
    """Every point within hgs (+ one ulp) of the centre of the cell its index names; its time inside its slice."""
    import raymarching
    H3 = H ** 3
    idx = indices.cpu().numpy().astype(np.int64)
    assert (idx >= 0).all() and (idx < T * C * H3).all()
    seg, cell = idx // H3, idx % H3
    t, cas = seg // C, seg % C
    coords = raymarching.morton3D_invert(torch.from_numpy(cell.astype(np.int32)).to(indices.device)).cpu().numpy()
    assert np.array_equal(coords, dh.morton3_invert(cell))
    p = xyzs.cpu().numpy().astype(np.float64)
    for c in range(C):
        m = cas == c
        centre, hgs = dh.cell_centre64(coords[m], c, H, bound)
        ulp = float(np.spacing(np.float32(min(2 ** c, bound))))
        assert np.abs(p[m] - centre).max() <= hgs + ulp
    tm = times.cpu().numpy()
    lo, hi = dh.slice_bounds32(t, T)
    assert (tm >= lo).all() and (tm <= hi).all()
    return t, cas, cell


@pytest.mark.parametrize("T,C,H,bound", [(1, 1, 2, 1), (3, 2, 8, 2), (4, 1, 8, 1)])
def test_full_points(cuda, T, C, H, bound):
    import dnerf
    P = T * C * H ** 3
    xyzs, times, indices = dnerf.grid_points(None, T, C, H, bound, False, 5, 0, 0, P)
    assert torch.equal(indices, torch.arange(P, dtype=torch.int32, device=cuda))  # point p is cell p
    t, cas, cell = _check_points(xyzs, times, indices, T, C, H, bound)
    rows = np.arange(P)
    assert np.array_equal(t, rows // (C * H ** 3)) and np.array_equal(cas, rows // H ** 3 % C)
    # the jitter is not degenerate: positions and times vary inside the cells
    if P >= 512:
        assert times.unique().numel() > P // 2 and xyzs.unique().numel() > P
    # a range not on multiples of 64 is that slice of the whole
    lo, hi = (3, 7) if P == 8 else (67, P - 33)
    a, b, c = dnerf.grid_points(None, T, C, H, bound, False, 5, 0, lo, hi)
    assert torch.equal(a, xyzs[lo:hi]) and torch.equal(b, times[lo:hi]) and torch.equal(c, indices[lo:hi])
    # the same (seed, update): the same bits; another update or seed: other noise, the same cells
    a, b, c = dnerf.grid_points(None, T, C, H, bound, False, 5, 0, 0, P)
    assert torch.equal(a, xyzs) and torch.equal(b, times) and torch.equal(c, indices)
    for seed, update in ((5, 1), (6, 0)):
        a, b, c = dnerf.grid_points(None, T, C, H, bound, False, seed, update, 0, P)
        assert not torch.equal(a, xyzs) and not torch.equal(b, times) and torch.equal(c, indices)
    # an empty range is a no-op
    assert dnerf.grid_points(None, T, C, H, bound, False, 5, 0, 4, 4)[0].shape == (0, 3)


def test_partial_points(cuda):
    import dnerf
    T, C, H, bound = 3, 2, 8, 2
    H3, N = H ** 3, H ** 3 // 4
    grid = torch.zeros(T, C, H3, device=cuda)
    occupied = [5, 100, 511]
    grid[0, 0, occupied] = torch.tensor([0.5, 1e-6, 3.0], device=cuda)  # slice 0 cascade 0: three cells
    grid[0, 0, 7] = -1.0                                               # (an untrained cell is not occupied)
    grid[1] = 1.0                                                      # slice 1: every cell
    grid[2] = -1.0                                                     # slice 2: none (slice 0 cascade 1: zeros)
    ws = dnerf.grid_points_workspace(T, C, H, cuda)
    P = T * C * 2 * N
    before = grid.clone()
    xyzs, times, indices = dnerf.grid_points(grid, T, C, H, bound, True, 11, 16, 0, P, ws)
    assert torch.equal(grid, before)  # the grid is only read
    t, cas, cell = _check_points(xyzs, times, indices, T, C, H, bound)
    seg = np.arange(P) // (2 * N)
    assert np.array_equal(t * C + cas, seg)  # every index lies in its segment (empty segments included)
    cell = cell.reshape(T * C, 2, N)
    # the occupied half of slice 0 cascade 0 draws only its three cells, and each of them
    assert sorted(set(cell[0, 1].tolist())) == occupied
    # slice 1: any cell may come; empty segments draw uniformly: many distinct cells in both halves
    for s in range(T * C):
        assert len(set(cell[s, 0].tolist())) >= 64  # ~113 of 512 expected from 128 uniform draws
        if s != 0:
            assert len(set(cell[s, 1].tolist())) >= 64
    # ranges (here across a segment and a half boundary) are slices of the whole; the draw is deterministic
    for lo, hi in ((0, P), (130, 700), (255, 257), (1300, P)):
        a, b, c = dnerf.grid_points(grid, T, C, H, bound, True, 11, 16, lo, hi, ws)
        assert torch.equal(a, xyzs[lo:hi]) and torch.equal(b, times[lo:hi]) and torch.equal(c, indices[lo:hi])
    c2 = dnerf.grid_points(grid, T, C, H, bound, True, 11, 17, 0, P, ws)[2]
    assert not torch.equal(c2, indices)
    # a partial update needs the grid and the workspace
    with pytest.raises(RuntimeError, match="workspace"):
        dnerf.grid_points(grid, T, C, H, bound, True, 11, 16, 0, P, None)
    with pytest.raises(RuntimeError, match="workspace"):
        dnerf.grid_points(grid, T, C, H, bound, True, 11, 16, 0, P, ws[:64])


def test_points_argument_errors(cuda):
    import _ngp_native as nat
    lib = nat.lib()
    buf = torch.zeros(64, device=cuda)
    p = buf.data_ptr()
    for T, C, H in ((1, 1, 6), (0, 1, 8), (1, 17, 8), (1025, 1, 8), (1024, 16, 1024)):
        assert lib.ngp_dnerf_grid_points(None, T, C, H, 1.0, 0, 0, 0, 0, 1, None, 0, p, p, p, None) == ARG_ERROR
        assert lib.ngp_dnerf_grid_points_workspace_bytes(T, C, H) == 0
    assert lib.ngp_dnerf_grid_points(None, 1, 1, 2, 1.0, 0, 0, 0, 0, 9, None, 0, p, p, p, None) == ARG_ERROR  # hi > P
    assert lib.ngp_dnerf_grid_points(None, 1, 1, 2, 1.0, 0, 0, 0, 5, 4, None, 0, p, p, p, None) == ARG_ERROR  # lo > hi
    assert b"outside" in lib.ngp_last_error()


# ---- ema, mean, pack --------------------------------------------------------------------
def _ema_case(seed=0):
    """(3, 2, 8): -1, 0, values on both sides of the threshold 0.25 and one exactly on it; tmp -1 and values."""
    rng = np.random.default_rng(seed)
    grid = rng.choice(np.array([-1.0, 0.0, 0.1, 0.2, 0.26, 0.9, 3.0], np.float32), size=(3, 2, 512))
    tmp = np.where(rng.random((3, 2, 512)) < 0.5, -1.0, rng.random((3, 2, 512)) * 2).astype(np.float32)
    grid[1, 1, 17], tmp[1, 1, 17] = 0.25, -1.0         # stays exactly on the threshold
    grid[2, 0, 40], tmp[2, 0, 40] = 0.5, 0.25          # max(0.5 * 0.5, 0.25) = 0.25: on it after the EMA
    grid[0, 0, 3], tmp[0, 0, 3] = 0.0, 0.0
    return grid.astype(np.float32), tmp


def test_ema_pack_against_restatement(cuda):
    import dnerf
    T, C, H = 3, 2, 8
    grid, tmp = _ema_case()
    want_g, want_t, want_sum, want_mean, want_bits = dh.ema_pack_ref(grid, tmp, 0.5, 0.25)
    assert float(want_mean) > 0.25  # the threshold is density_thresh here
    g, t = torch.from_numpy(grid).to(cuda), torch.from_numpy(tmp).to(cuda)
    bits = torch.full((T, C * H ** 3 // 8), 0xAA, dtype=torch.uint8, device=cuda)
    stats = dnerf.grid_ema_pack(g, t, T, C, H, 0.5, 0.25, bits)
    assert np.array_equal(g.cpu().numpy().view(np.uint32), want_g.view(np.uint32))
    assert (t == -1).all()
    assert stats[0].item() == pytest.approx(want_sum, rel=1e-12)
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert g[1, 1, 17].item() == 0.25 and g[2, 0, 40].item() == 0.25
    assert not (int(want_bits[1, (512 + 17) // 8]) >> ((512 + 17) % 8)) & 1  # on the threshold: not occupied
    # a second pass on the reset tmp: nothing to blend, the same grid and bits
    stats2 = dnerf.grid_ema_pack(g, t, T, C, H, 0.5, 0.25, bits)
    assert np.array_equal(g.cpu().numpy().view(np.uint32), want_g.view(np.uint32))
    assert stats2[0].item() == stats[0].item() and np.array_equal(bits.cpu().numpy(), want_bits)
    # the smallest grid
    g1 = np.array([[[0.5, -1, 0.0, 2.0, 0.3, 0.1, 0.0, 1.0]]], np.float32)
    t1 = np.array([[[1.0, 0.5, -1, 0.0, 0.1, 0.2, 0.0, -1]]], np.float32)
    w = dh.ema_pack_ref(g1, t1, 0.95, 0.3)
    a, b = torch.from_numpy(g1).to(cuda), torch.from_numpy(t1).to(cuda)
    bits1 = torch.zeros(1, 1, dtype=torch.uint8, device=cuda)
    s1 = dnerf.grid_ema_pack(a, b, 1, 1, 2, 0.95, 0.3, bits1)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), w[0].view(np.uint32)) and bits1.item() == w[4][0, 0]
    assert s1[0].item() == pytest.approx(w[2], rel=1e-12)


def test_ema_pack_thresholds_at_the_global_mean(cuda):
    """The global mean is below density_thresh while slice 1's own mean is above the global one: slice 1's bits
    differ from what the single-grid entry gives on that slice alone."""
    import _ngp_native as nat
    import dnerf
    T, C, H = 3, 2, 8
    grid = np.zeros((T, C, 512), np.float32)
    grid[1] = np.random.default_rng(1).choice(np.array([0.5, 1.5], np.float32), size=(C, 512))  # mean ~1
    tmp = np.full_like(grid, -1.0)
    want = dh.ema_pack_ref(grid, tmp, 0.95, 10.0)
    slice_mean = float(grid[1].mean())
    assert float(want[3]) < 0.5 < slice_mean < 10.0  # global ~1/3, slice 1's own ~1
    g, t = torch.from_numpy(grid).to(cuda), torch.from_numpy(tmp).to(cuda)
    bits = torch.zeros(T, C * 512 // 8, dtype=torch.uint8, device=cuda)
    dnerf.grid_ema_pack(g, t, T, C, H, 0.95, 10.0, bits)
    assert np.array_equal(bits.cpu().numpy(), want[4])
    assert (bits[1] == 0xFF).all() and (bits[0] == 0).all() and (bits[2] == 0).all()  # 0.5 and 1.5 > 1/3
    # the single-grid entry on slice 1 alone thresholds at that slice's mean: the 0.5 cells drop out
    g1, t1 = g[1].clone(), torch.full_like(g[1], -1.0)
    one = torch.zeros(C * 512 // 8, dtype=torch.uint8, device=cuda)
    stats = torch.empty(nat.DENSITY_STATS_LEN, dtype=torch.float64, device=cuda)
    nat.check(nat.lib().ngp_density_grid_ema_pack(g1.data_ptr(), t1.data_ptr(), C, H, 0.95, 10.0, stats.data_ptr(),
                                                  one.data_ptr(), None), "density_grid_ema_pack")
    assert not torch.equal(one, bits[1]) and not (one == 0xFF).all()


def test_ema_pack_nan_clears_every_bit(cuda):
    import dnerf
    T, C, H = 3, 2, 8
    grid, tmp = _ema_case(1)
    grid[1, 0, 9] = np.nan
    g, t = torch.from_numpy(grid).to(cuda), torch.from_numpy(tmp).to(cuda)
    bits = torch.full((T, C * 512 // 8), 0xFF, dtype=torch.uint8, device=cuda)
    stats = dnerf.grid_ema_pack(g, t, T, C, H, 0.5, 0.25, bits)
    assert torch.isnan(stats[0]).item() and (bits == 0).all()
    assert np.array_equal(bits.cpu().numpy(), dh.ema_pack_ref(grid, tmp, 0.5, 0.25)[4])


def test_ema_pack_argument_errors(cuda):
    import _ngp_native as nat
    lib = nat.lib()
    buf = torch.zeros(2048, dtype=torch.float64, device=cuda)
    p = buf.data_ptr()
    for T, C, H in ((1, 1, 6), (1, 1, 1), (0, 1, 8), (1024, 16, 1024), (1, 1, 2048)):
        assert lib.ngp_dnerf_grid_ema_pack(p, p, T, C, H, 0.95, 0.01, p, p, None) == ARG_ERROR
        assert b"out of range" in lib.ngp_last_error()
    assert lib.ngp_dnerf_grid_ema_pack(None, p, 1, 1, 2, 0.95, 0.01, p, p, None) == ARG_ERROR


# ---- update_extra_state ------------------------------------------------------------------
def _small_model(cuda, **kw):
    from dnerf import NeRFNetwork
    torch.manual_seed(0)
    args = dict(bound=1, time_size=2, grid_size=8, density_thresh=0.01)
    args.update(kw)
    m = NeRFNetwork(**args).to(cuda)
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-0.5, 0.5)  # densities that vary from cell to cell
    return m


def test_update_extra_state_against_torch(cuda):
    """One full and one partial update equal, bit for bit, a torch restatement that consumes the kernel's own
    points, times and indices; an update past iter_density = 100 queries nothing and blends nothing."""
    m = _small_model(cuda)
    m.grid_seed = 3
    m.density_grid[0, 0, 5] = -1.0   # an untrained cell stays -1
    m.density_grid[1, 0, 9] = 50.0   # decays: 50 * 0.95 beats any density here
    want, want_mean = dh.update_reference(m)
    m.update_extra_state()
    assert torch.equal(m.density_grid, want) and m.iter_density == 1
    assert m.density_grid[0, 0, 5].item() == -1.0 and m.density_grid[1, 0, 9].item() == np.float32(50.0) * np.float32(0.95)
    assert m.mean_density == want_mean and (m._tmp_grid == -1).all()
    thresh = min(m.mean_density, m.density_thresh)
    import raymarching
    for t in range(2):
        assert torch.equal(m.density_bitfield[t], raymarching.packbits(m.density_grid[t], thresh))
    assert m.density_bitfield.any()
    # partial: thin the grid out so that the occupied draw matters
    m.iter_density = 16
    m.density_grid[0, 0, 64:] = 0.0
    want, want_mean = dh.update_reference(m)
    m.update_extra_state()
    assert torch.equal(m.density_grid, want) and m.mean_density == want_mean and m.iter_density == 17
    assert (m.density_grid[0, 0, :64] > 0).sum() > 32
    # past 100: no query, tmp stays -1, so no cell is blended; the mean and bits are recomputed
    m.iter_density = 100
    calls = []
    orig = m.density
    m.density = lambda *a, **k: calls.append(1) or orig(*a, **k)
    before = m.density_grid.clone()
    m.update_extra_state()
    assert not calls and torch.equal(m.density_grid, before) and m.iter_density == 101
    assert m.mean_density == want_mean


def test_update_extra_state_mean_count(cuda):
    m = _small_model(cuda)
    m.step_counter[:3, 0] = torch.tensor([10, 20, 31], dtype=torch.int32, device=cuda)
    m.local_step = 3
    m.update_extra_state()
    assert m.mean_count == 20 and m.local_step == 0


# ---- network --------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row_time", [False, True])
def test_network_forward_is_the_composition(cuda, per_row_time):
    m = _small_model(cuda)
    N = 257
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(N, 3, generator=g) * 2 - 1).to(cuda)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(cuda)
    t = torch.rand(N if per_row_time else 1, 1, generator=g).to(cuda)
    sigma, rgbs, deform = m(x, d, t)
    ws, wr, wd = dh.compose_forward(m, x, d, t)
    assert sigma.shape == (N,) and rgbs.shape == (N, 3) and deform.shape == (N, 3)
    assert torch.equal(sigma, ws) and torch.equal(rgbs, wr) and torch.equal(deform, wd)
    dens = m.density(x, t)
    assert torch.equal(dens["sigma"], ws) and torch.equal(dens["deform"], wd) and dens["geo_feat"].shape == (N, 15)
    assert torch.equal(m.color(x, d, geo_feat=dens["geo_feat"]), wr)
    mask = torch.arange(N, device=cuda) % 3 == 0
    masked = m.color(x, d, mask=mask, geo_feat=dens["geo_feat"])
    assert torch.equal(masked[mask], m.color(x[mask], d[mask], geo_feat=dens["geo_feat"][mask]))
    assert (masked[~mask] == 0).all()
    # the deformation trains through the grid's input gradient (sigma and rgbs see deform only there)
    (sigma.sum() + rgbs.sum()).backward()
    grads = [layer.weight.grad for layer in m.deform_net]
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)
    assert any(gr.abs().sum().item() > 0 for gr in grads)
    assert m.encoder.embeddings.grad.abs().sum().item() > 0


# ---- training ---------------------------------------------------------------------------------
def _train(cuda, scene, freeze_time, steps=300):
    from dnerf import DNeRFTrainer, NeRFDataset, NeRFNetwork, seed_everything
    seed_everything(0)
    data = NeRFDataset(scene, cuda, type="train", scale=dh.SCENE_SCALE, num_rays=1024, store="uint8")
    if freeze_time:
        data.times.fill_(0.5)
    model = NeRFNetwork(bound=1, time_size=4, grid_size=32, density_thresh=10).to(cuda)
    trainer = DNeRFTrainer(model, data, iters=steps, dt_gamma=0, max_steps=256, log=None)
    model.train()
    model.mark_untrained_grid(data.poses, data.intrinsics)
    with torch.autocast("cuda", dtype=torch.float16):
        model.update_extra_state()  # a first occupancy grid, so that the untrained field is rendered too
    before = dh.scene_mse(model, data)
    trainer.train()
    return before, dh.scene_mse(model, data), model, data


def test_training_learns_the_motion(cuda, tmp_path, parity_report):
    """A sphere moving along x, 8 poses x 4 times at 32 x 32; time_size 4, 300 steps of 1024 rays: the final
    training MSE is below the untrained one and below that of a control run with every frame's time at 0.5."""
    scene = dh.write_scene(str(tmp_path / "scene"))
    before, after, model, data = _train(cuda, scene, False)
    _, control, _, _ = _train(cuda, scene, True)
    print(f"dnerf training: mse before {before:.6f} after {after:.6f} control (time 0.5) {control:.6f}")
    parity_report(f"mse before {before:.6f} after {after:.6f} control {control:.6f}")
    assert data.times.unique().numel() == 4 and model.iter_density == 4
    assert np.isfinite(after) and after < before
    assert after < control


# ---- front door ---------------------------------------------------------------------------------
def test_main_dnerf_trains_saves_and_tests(cuda, tmp_path):
    import main_dnerf
    scene = dh.write_scene(str(tmp_path / "scene"))
    ws = str(tmp_path / "ws")
    argv = [scene, "-O", "--iters", "50", "--workspace", ws, "--bound", "1", "--scale", str(dh.SCENE_SCALE),
            "--dt_gamma", "0", "--max_steps", "256", "--num_rays", "1024", "--time_size", "4", "--grid_size", "32"]
    out = main_dnerf.main(argv)
    assert os.path.exists(os.path.join(ws, "checkpoints", "ngp.pth")) and np.isfinite(out["psnr"])
    names = sorted(os.listdir(os.path.join(ws, "results")))
    assert names == sorted(f"ngp_{i:04d}_{k}.png" for i in range(4) for k in ("rgb", "depth"))
    from PIL import Image
    assert Image.open(os.path.join(ws, "results", "ngp_0000_rgb.png")).size == (32, 32)
    for n in names:
        os.remove(os.path.join(ws, "results", n))
    out2 = main_dnerf.main(argv + ["--test"])
    assert sorted(os.listdir(os.path.join(ws, "results"))) == names and len(out2["files"]) == 8
