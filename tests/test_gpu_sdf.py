"""GPU: the SDF family (csrc/sdf.hip, sdf/, main_sdf.py) against the numpy
references of tests/sdf_helpers.py, which tests/test_sdf_cpu.py holds to the
winding number and the analytic box.

No reference run is possible (trimesh and pysdf are absent), so the training
test compares against a plain torch trainer on host-made batches."""
import os

import numpy as np
import pytest
import torch

import sdf
import sdf_helpers as sh
from sdf.provider import new_counter, prepare_mesh, sdf_query, sdf_sample

pytestmark = pytest.mark.gpu

_MESH, _REF = {}, {}


def mesh_of(name, dev):
    if name not in _MESH:
        _MESH[name] = prepare_mesh(*sh.MESHES[name](), device=dev)
    return _MESH[name]


def corners32(m):
    """The float32 corners the kernels read, as float64 vertices."""
    return m.vertices.astype(np.float32).astype(np.float64)


def reference(name, dev):
    """(points f32 [1000, 3], float64 signed distance) of a mesh, computed once."""
    if name not in _REF:
        m = mesh_of(name, dev)
        pts = sh.query_points(m.vertices, m.faces)
        _REF[name] = (pts, sh.signed_distance(corners32(m), m.faces, pts)[0])
    return _REF[name]


# ---- 1. the query against float64 -----------------------------------------------

@pytest.mark.parametrize("name", list(sh.MESHES))
def test_query_against_float64(cuda, name):
    """Distance within sh.DIST_BOUND = 4.08e-7 (4 x the float32 restatement's
    largest error on these very points, 1.018e-7, measured on the CPU by
    tests/test_sdf_cpu.py) of the float64 brute force; equal signs wherever
    |d64| is above the bound; at most 2 % of the points below it."""
    m = mesh_of(name, cuda)
    assert m.T == sh.FACES[name]
    pts, d64 = reference(name, cuda)
    for n in (1, 63, 64, 65, 1000):
        p = torch.from_numpy(pts[:n]).to(cuda)
        for cull in (False, True):
            d, feat = sdf_query(m, p, cull=cull, feature=True)
            d, feat = d.cpu().numpy().astype(np.float64), feat.cpu().numpy()
            err = np.abs(np.abs(d) - np.abs(d64[:n])).max()
            near = np.abs(d64[:n]) <= sh.DIST_BOUND
            print(f"{name} n={n} cull={cull}: max | |d| - |d64| | = {err:.3e}, below the bound {int(near.sum())}")
            assert err <= sh.DIST_BOUND
            assert np.array_equal(d[~near] < 0, d64[:n][~near] < 0)
            assert near.sum() <= 0.02 * n
            assert feat.min() >= 0 and (feat >> 3).max() < m.T and (feat & 7).max() <= 6


def test_query_empty_and_argument_checks(cuda):
    m = mesh_of("cube", cuda)
    assert sdf_query(m, torch.empty(0, 3, device=cuda)).shape == (0,)
    with pytest.raises(RuntimeError, match="CUDA"):
        sdf_query(m, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="one entry per point"):
        sdf_query(m, torch.zeros(4, 3, device=cuda), tri=torch.zeros(3, dtype=torch.int32, device=cuda))
    # a start triangle outside [0, T) is no start
    p = torch.from_numpy(reference("cube", cuda)[0][:64]).to(cuda)
    bad = torch.full((64,), 12, dtype=torch.int32, device=cuda)
    bad[::2] = -7
    assert torch.equal(sdf_query(m, p, tri=bad), sdf_query(m, p))


# ---- 2. culled against plain ----------------------------------------------------

@pytest.mark.parametrize("name", ["bipyramid_66", "torus_96", "torus_1024", "two_cubes"])
def test_cull_equals_plain_bit_for_bit(cuda, name):
    m = mesh_of(name, cuda)
    p = torch.from_numpy(reference(name, cuda)[0]).to(cuda)
    a, fa = sdf_query(m, p, cull=False, feature=True)
    b, fb = sdf_query(m, p, cull=True, feature=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(fa, fb)
    # with start triangles: the batch's second half, perturbed points and uniform ones (tri -1)
    N = 4096
    pts, tri = sdf_sample(m, N, 7, new_counter(cuda, 3))
    q, t = pts[N // 2:].contiguous(), tri[N // 2:].contiguous()
    assert int((t >= 0).sum()) == 3 * N // 8 and int((t == -1).sum()) == N // 8
    c, fc = sdf_query(m, q, tri=t, cull=False, feature=True)
    d, fd = sdf_query(m, q, tri=t, cull=True, feature=True)
    assert torch.equal(c.view(torch.int32), d.view(torch.int32)) and torch.equal(fc, fd)
    # the start changes no distance: the minimum is over the same faces
    e = sdf_query(m, q, cull=True)
    assert torch.equal(e.abs().view(torch.int32), d.abs().view(torch.int32))
    far = e.abs() > sh.DIST_BOUND
    assert torch.equal(e[far] < 0, d[far] < 0)


# ---- 3. the sampler -----------------------------------------------------------------

@pytest.mark.parametrize("name,N", [("torus_96", 8), ("torus_96", 64), ("torus_96", 4096), ("torus_1024", 4096),
                                    ("bipyramid_66", 64)])
def test_sampler_against_restatement(cuda, name, N):
    m = mesh_of(name, cuda)
    seed, step = 1234, 5
    counter = new_counter(cuda, step)
    p1, t1 = sdf_sample(m, N, seed, counter)
    p1, t1 = p1.clone(), t1.clone()
    assert counter.cpu().tolist() == [step + 1, 0]
    p2, t2 = sdf_sample(m, N, seed, counter)
    assert counter.cpu().tolist() == [step + 2, 0]
    assert not torch.equal(p1, p2)
    p3, t3 = sdf_sample(m, N, seed, new_counter(cuda, step))
    assert torch.equal(p1.view(torch.int32), p3.view(torch.int32)) and torch.equal(t1, t3)
    ref_p, ref_t = sh.sample_f32(m.tris.cpu().numpy(), m.cdf.cpu().numpy(), N, seed, step)
    ref_p2, _ = sh.sample_f32(m.tris.cpu().numpy(), m.cdf.cpu().numpy(), N, seed, step + 1)
    got, got_t = p1.cpu().numpy(), t1.cpu().numpy()
    h, u = N // 2, N // 8 * 7
    assert np.array_equal(got_t, ref_t) and np.all(got_t[u:] == -1) and np.all(got_t[:u] >= 0)
    assert np.abs(got[:h] - ref_p[:h]).max() <= 1e-6
    # 0.01 |z| <= 0.06 at a few ulps of libm's log and cos, and one rounding of a coordinate <= 1
    assert np.abs(got[h:u] - ref_p[h:u]).max() <= 1e-6
    assert np.array_equal(got[u:].view(np.uint32), ref_p[u:].view(np.uint32))
    assert np.abs(p2.cpu().numpy() - ref_p2).max() <= 1e-6
    # the first half lies on its triangle: the float64 distance to it is rounding
    tris = m.tris.cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    d2, _, _ = sh.closest(got[:h].astype(np.float64), tris, np.float64)
    assert np.sqrt(d2[np.arange(h), got_t[:h]]).max() <= 1e-6


def test_sampler_refuses_bad_size(cuda):
    m = mesh_of("torus_96", cuda)
    counter = new_counter(cuda, 0)
    with pytest.raises(RuntimeError, match="divisible by 8"):
        sdf_sample(m, 12, 0, counter)
    assert counter.cpu().tolist() == [0, 0]


def test_sampler_area_weighting(cuda):
    """Triangle frequencies follow the areas (a chi-square at 5 sigma of its own spread)."""
    m = mesh_of("bipyramid_66", cuda)
    N = 2 ** 16
    _, tri = sdf_sample(m, N, 3, new_counter(cuda))
    counts = np.bincount(tri.cpu().numpy()[:N // 8 * 7], minlength=m.T).astype(np.float64)
    cdf = m.cdf.cpu().numpy().astype(np.float64)
    expect = np.diff(np.concatenate([[0.0], cdf])) * (N // 8 * 7)
    chi2 = ((counts - expect) ** 2 / expect).sum()
    assert chi2 <= (m.T - 1) + 5 * np.sqrt(2 * (m.T - 1))


# ---- 4. the loss ------------------------------------------------------------------------

def _mape_torch(pred, y):
    return (torch.abs(pred - y) / (torch.abs(y) + 1e-2)).mean()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mape_loss_and_gradient(cuda, n):
    g = torch.Generator().manual_seed(n)
    y = (torch.randn(n, generator=g) * 0.3)
    pred = (torch.randn(n, generator=g) * 0.3)
    y[::3] = 0.0  # targets on the surface
    if n > 4:
        pred[4] = y[4]  # a zero residual: sign 0
    y, pred = y.to(cuda), pred.to(cuda)
    ref64 = _mape_torch(pred.double(), y.double())
    leaf = pred.clone().requires_grad_(True)
    _mape_torch(leaf, y).backward()
    loss, grad = sdf.mape(pred, y)
    assert loss.dtype == torch.float64 and grad.dtype == torch.float32
    assert abs(loss.item() - ref64.item()) <= 1e-12 * abs(ref64.item())
    assert torch.equal(grad, leaf.grad), (grad - leaf.grad).abs().max().item()
    # fp16: the gradient within one fp16 ulp of torch's on the same values
    p16 = pred.half()
    leaf = p16.float().requires_grad_(True)
    _mape_torch(leaf, y).backward()
    loss16, g16 = sdf.mape(p16, y)
    assert g16.dtype == torch.float16
    ref = leaf.grad.double()
    ulp = torch.clamp(2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 10), min=2.0 ** -24)
    assert bool(((g16.double() - ref).abs() <= ulp).all())
    r16 = _mape_torch(p16.double(), y.double()).item()
    assert abs(loss16.item() - r16) <= 1e-12 * abs(r16)
    # the autograd op: the incoming gradient multiplies before the rounding
    leaf = pred.clone().requires_grad_(True)
    out = sdf.mape_loss(leaf.view(-1, 1), y.view(-1, 1))
    assert out.dtype == torch.float32 and out.item() == pytest.approx(ref64.item(), rel=1e-6)
    (out * 128.0).backward()
    assert torch.equal(leaf.grad, grad * 128.0)
    # two runs: the same bits
    assert sdf.mape(pred, y)[0].item() == loss.item()


# ---- 5. the exact volume ---------------------------------------------------------------------

def test_exact_volume_round_trip(cuda):
    from nerf.mesh import marching_cubes
    m = mesh_of("torus_96", cuda)
    R = 48
    out = []
    for _ in range(2):
        vol = sdf.mesh_sdf_volume(m, R, chunk=40000)  # three chunks
        assert vol.shape == (R, R, R) and vol.dtype == torch.float32
        v, f = marching_cubes(-vol, 0.0, aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
        out.append((v.cpu().numpy(), f.cpu().numpy()))
    (v, f), (v2, f2) = out
    assert len(v) > 0 and len(f) > 0
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()
    # the field is 1-Lipschitz and a true zero lies on the vertex's lattice edge
    d64, _, _ = sh.signed_distance(corners32(m), m.faces, v.astype(np.float64))
    print(f"volume round trip: {len(v)} vertices, max |sdf| {np.abs(d64).max():.4f}, h {2 / (R - 1):.4f}")
    assert np.abs(d64).max() <= 2 / (R - 1)
    # the lattice itself against float64 on a sample of its points
    idx = np.random.default_rng(0).integers(0, R, (500, 3))
    pts = (-1 + 2 * idx / (R - 1)).astype(np.float32)
    ref, _, _ = sh.signed_distance(corners32(m), m.faces, pts)
    got = vol[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-6


# ---- 6. training -----------------------------------------------------------------------------

TRAIN_STEPS, TRAIN_N = 300, 2 ** 12
# The allowed ratio over the yardstick, from the yardstick's own spread. Its
# error over the data seeds 0, 1, 2, measured twice on an MI355X: 0.059614,
# 0.059547, 0.059598 and 0.059586, 0.059567, 0.059510 (the same seed differs
# between runs: the grid backward accumulates with atomics), max / min 1.0018.
# The test divides one such draw by another, so the ratio's own spread is that
# squared, 1.0036; the allowed ratio is just above it. The device trainer's
# errors in the same runs: 0.059503 .. 0.059649. DESIGN.md §21,
# profiles/sdf_bench.json.
YARDSTICK_RATIO = 1.005


def _small_net(dev):
    torch.manual_seed(0)
    return sdf.SDFNetwork(encoding="hashgrid", log2_hashmap_size=14).to(dev)


def _eval_set(m):
    pts, _ = sh.sample_f32(m.tris.cpu().numpy(), m.cdf.cpu().numpy(), 4096, 99, 10000)
    return pts, sh.signed_distance(corners32(m), m.faces, pts)[0]


def yardstick_error(m, dev, seed, steps=TRAIN_STEPS, N=TRAIN_N, lr=1e-4):
    """A plain torch trainer: host-made batches (the sampler's restatement, the
    float64 signed distance), mape written in torch, torch.optim.Adam with the
    trainer's settings -> mean |pred - sdf64| on the evaluation set."""
    tris, cdf = m.tris.cpu().numpy(), m.cdf.cpu().numpy()
    v, f = corners32(m), m.faces
    model = _small_net(dev)
    opt = torch.optim.Adam([{"params": list(model.encoder.parameters())},
                            {"params": list(model.backbone.parameters()), "weight_decay": 1e-6}],
                           lr=lr, betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    model.train()
    for step in range(steps):
        pts, _ = sh.sample_f32(tris, cdf, N, seed, step)
        y = np.zeros(N, np.float32)
        y[N // 2:] = sh.signed_distance(v, f, pts[N // 2:])[0]
        x, t = torch.from_numpy(pts).to(dev), torch.from_numpy(y).to(dev).view(-1, 1)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            pred = model(x)
        loss = _mape_torch(pred.float(), t)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    return _error(model, m, dev)


def _error(model, m, dev):
    pts, d64 = _eval_set(m)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        pred = model(torch.from_numpy(pts).to(dev)).float().reshape(-1).cpu().numpy()
    return float(np.abs(pred - d64).mean())


def device_error(m, dev, seed, steps=TRAIN_STEPS, N=TRAIN_N, lr=1e-4):
    model = _small_net(dev)
    w0 = [p.detach().clone() for p in model.parameters()]
    tr = sdf.SDFTrainer(model, sdf.SDFDataset(m, num_samples=N, seed=seed), lr=lr)
    losses = torch.stack([tr.train_step() for _ in range(steps)])
    assert bool(torch.isfinite(losses).all())
    assert all(not torch.equal(a, b.detach()) for a, b in zip(w0, model.parameters()))
    assert tr.dataset.counter.cpu().tolist() == [steps, 0]
    return _error(model, m, dev), losses


def test_training_against_torch_yardstick(cuda):
    """300 steps at N = 2^12 on the 96-face torus: the device trainer's mean
    |pred - sdf64| on 4,096 float64-signed points is at most YARDSTICK_RATIO x
    the plain torch trainer's."""
    m = mesh_of("torus_96", cuda)
    ref = yardstick_error(m, cuda, seed=0)
    err, losses = device_error(m, cuda, seed=0)
    print(f"training: device {err:.6f}, yardstick {ref:.6f}, ratio {err / ref:.4f}; "
          f"loss {losses[0].item():.4f} -> {losses[-10:].mean().item():.4f}")
    assert err <= YARDSTICK_RATIO * ref


def test_dataset_layout_and_clip(cuda):
    m = mesh_of("torus_96", cuda)
    N = 4096
    for sort in (False, True):
        ds = sdf.SDFDataset(m, num_samples=N, seed=2, sort=sort)
        b = ds.sample()
        pts, y = b["points"].cpu().numpy(), b["sdfs"].cpu().numpy()
        assert pts.shape == (N, 3) and y.shape == (N, 1) and np.all(y[:N // 2] == 0)
        d64, _, _ = sh.signed_distance(corners32(m), m.faces, pts[N // 2:])
        assert np.abs(np.abs(y[N // 2:, 0]) - np.abs(d64)).max() <= sh.DIST_BOUND
        far = np.abs(d64) > sh.DIST_BOUND
        assert np.array_equal(y[N // 2:, 0][far] < 0, d64[far] < 0)
    clipped = sdf.SDFDataset(m, num_samples=N, seed=2, clip_sdf=0.05, sort=True).sample()["sdfs"].cpu().numpy()
    assert np.array_equal(clipped, np.clip(y, -0.05, 0.05))


# ---- 7. the command line -------------------------------------------------------------------------

def test_main_sdf_trains_and_tests(cuda, tmp_path):
    import main_sdf
    from nerf.mesh import read_ply
    obj, ws = str(tmp_path / "ico.obj"), str(tmp_path / "ws")
    sh.write_obj(obj, *sh.icosahedron())
    args = [obj, "--workspace", ws, "--fp16", "--ff", "--num_samples", "4096", "--epochs", "2",
            "--steps_per_epoch", "10", "--mesh_resolution", "32", "--lr", "1e-3"]
    tr = main_sdf.main(args)
    assert tr.global_step == 20 and tr.epoch == 2
    ply = os.path.join(ws, "results", "output.ply")
    assert os.path.getsize(os.path.join(ws, "checkpoints", "ngp.pth")) > 0
    v, f, _ = read_ply(ply)
    assert len(v) > 0 and len(f) > 0 and np.abs(v).max() <= 1.0
    first = open(ply, "rb").read()
    os.remove(ply)
    main_sdf.main(args + ["--test"])
    assert open(ply, "rb").read() == first
