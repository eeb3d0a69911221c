"""GPU: mesh export (csrc/mesh.hip, nerf/mesh.py, FusedTrainer.save_mesh,
main_nerf --save_mesh).

The marching-cubes tests run on synthetic volumes. The reference is a numpy
restatement of the vertex rule only (mesh_helpers.crossed_edges / vertex_rule:
which lattice edges are crossed, in (p, axis) order, and the fp32 interpolation
on each); the triangles are checked through what must hold of them whatever
the table: indices in range, every triangle on three edges of the cell it was
emitted for, cells in order, per-cell counts equal to the generated table's,
and on closed fields a closed, outward-oriented manifold."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mesh_helpers as mh

pytestmark = pytest.mark.gpu


def _mc(cuda, vol, thr, **kw):
    from nerf.mesh import marching_cubes
    out = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(cuda), thr, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_rule(vol, thr, verts, faces):
    """The vertex rule bit for bit, and the triangle structure."""
    shape = vol.shape
    nx, ny, nz = shape
    p, axis, _ = mh.crossed_edges(vol, thr)
    assert verts.shape == (len(p), 3) and verts.dtype == np.float32
    want = mh.vertex_rule(vol, thr, p, axis)
    assert np.array_equal(verts.view(np.uint32), want.view(np.uint32))
    assert faces.dtype == np.int32 and faces.ndim == 2 and faces.shape[1] == 3
    # the cell of every triangle, from the table's counts at the numpy case indices
    case = mh.case_index(vol, thr)
    counts = mh.tri_counts()[case]
    ii, jj, kk = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    cell_ijk = np.stack([ii, jj, kk], -1).reshape(-1, 3)  # ascending p
    assert faces.shape[0] == counts.sum()
    if not len(faces):
        return
    assert faces.min() >= 0 and faces.max() < len(p)
    tri_cell = np.repeat(cell_ijk, counts.reshape(-1), axis=0)  # [T, 3]
    # each corner of a triangle sits on lattice edge (q, a): q - cell in {0, 1}^3 with component a zero
    q = p[faces]  # [T, 3]
    a = axis[faces]
    q_ijk = np.stack([q // (ny * nz), q // nz % ny, q % nz], -1)  # [T, 3 corners, 3]
    rel = q_ijk - tri_cell[:, None, :]
    assert rel.min() >= 0 and rel.max() <= 1, "a triangle uses an edge outside its cell"
    assert np.all(np.take_along_axis(rel, a[..., None], -1) == 0)
    # the cell can also be read off the triangle alone (its edges' minimum point): nondecreasing along faces
    own = q_ijk.min(1)
    assert np.array_equal(own, tri_cell)
    own_p = (own[:, 0] * ny + own[:, 1]) * nz + own[:, 2]
    assert np.all(np.diff(own_p) >= 0)
    assert np.all((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))


@pytest.mark.parametrize("corner", range(8))
def test_single_corner_cases(cuda, corner):
    vol = np.zeros((2, 2, 2), np.float32)
    c = np.array([corner & 1, corner >> 1 & 1, corner >> 2])
    vol[tuple(c)] = 1.0
    verts, faces = _mc(cuda, vol, 0.25)
    _check_rule(vol, 0.25, verts, faces)
    assert verts.shape == (3, 3) and faces.shape == (1, 3)
    assert np.allclose(np.abs(verts - c).sum(1), 0.75)  # t = 0.25 or 0.75 along one axis from the corner
    t = verts[faces[0]].astype(np.float64)
    normal = np.cross(t[1] - t[0], t[2] - t[0])
    assert normal @ (t.mean(0) - c) > 0  # away from the inside corner
    # the complement: the same vertices, the triangle turned round
    verts2, faces2 = _mc(cuda, 1.0 - vol, 0.75)
    t2 = verts2[faces2[0]].astype(np.float64)
    assert np.cross(t2[1] - t2[0], t2[2] - t2[0]) @ (t2.mean(0) - c) < 0


def test_small_odd_noise(cuda):
    vol = np.random.default_rng(7).random((3, 5, 4), dtype=np.float32)
    verts, faces = _mc(cuda, vol, 0.5)
    _check_rule(vol, 0.5, verts, faces)
    assert len(verts) > 0 and len(faces) > 0


@pytest.mark.parametrize("seed", [0, 3])
def test_noise_16_closed_manifold(cuda, seed):
    vol = mh.noise_volume(seed)
    verts, faces = _mc(cuda, vol, 0.5)
    _check_rule(vol, 0.5, verts, faces)
    if seed == 0:
        assert len(verts) == 4496
    mh.assert_closed_manifold(faces, len(verts))
    assert mh.signed_volume(verts, faces) > 0
    # the CPU walker over the generated table gives the same index structure
    wv, wf = mh.walk(vol, 0.5)
    assert np.array_equal(wf, faces) and np.array_equal(wv.view(np.uint32), verts.view(np.uint32))


def test_nan_is_outside(cuda):
    vol = mh.noise_volume(1)
    vol[5, 6, 7] = np.nan
    vol[0, 0, 0] = np.nan
    verts, faces = _mc(cuda, vol, 0.5)
    _check_rule(vol, 0.5, verts, faces)
    assert np.isfinite(verts).all()


def test_sphere_odd_shape(cuda):
    vol = mh.sphere_volume((33, 17, 9))
    verts, faces = _mc(cuda, vol, 10.0)
    _check_rule(vol, 10.0, verts, faces)
    mh.assert_closed_manifold(faces, len(verts))
    assert mh.euler(faces) == 2


def test_sphere_65(cuda):
    """65^3 = 1073 blocks of 256 points: the block scan walks more than one block per thread."""
    shape = (65, 65, 65)
    vol = mh.sphere_volume(shape)
    verts, faces = _mc(cuda, vol, 10.0)
    _check_rule(vol, 10.0, verts, faces)
    mh.assert_closed_manifold(faces, len(verts))
    assert mh.euler(faces) == 2
    world = mh.lattice_to_world(verts, shape, (-1, -1, -1, 1, 1, 1)).astype(np.float64)
    r = mh.SPHERE_R
    dv = mh.signed_volume(world, faces) / (4 / 3 * np.pi * r ** 3) - 1
    da = mh.area(world, faces) / (4 * np.pi * r ** 2) - 1
    print(f"sphere 65^3: volume {dv:+.4%} area {da:+.4%}")
    assert abs(dv) < 0.03 and abs(da) < 0.03


@pytest.mark.parametrize("fill", [0.0, 20.0])
def test_empty_results_launch_no_emit(cuda, fill, monkeypatch):
    import _ngp_native as nat
    from nerf.mesh import marching_cubes

    def no_emit(*a):
        raise AssertionError("ngp_mesh_emit called for an empty mesh")
    monkeypatch.setattr(nat.lib(), "ngp_mesh_emit", no_emit)
    vol = torch.full((9, 6, 11), fill, device=cuda)
    v, f, n = marching_cubes(vol, 10.0, normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32


def test_two_runs_give_identical_bytes(cuda):
    vol = mh.noise_volume(2)
    a = _mc(cuda, vol, 0.5, normals=True, aabb=(-1, -1, -1, 1, 1, 1))
    b = _mc(cuda, vol, 0.5, normals=True, aabb=(-1, -1, -1, 1, 1, 1))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_normals_point_outward_on_the_sphere(cuda):
    vol = mh.sphere_volume((32, 32, 32))
    verts, faces, normals = _mc(cuda, vol, 10.0, normals=True, aabb=(-1, -1, -1, 1, 1, 1))
    assert normals.shape == verts.shape
    radial = verts.astype(np.float64) - mh.SPHERE_C
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (normals.astype(np.float64) * radial).sum(1)
    print(f"normal . radial: min {dots.min():.6f}")
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0, atol=1e-5)
    assert dots.min() >= 0.999


def test_aabb_maps_the_lattice_vertices(cuda):
    shape, aabb = (33, 17, 9), (-1.5, -0.5, 0.25, 2.0, 1.0, 3.0)
    vol = mh.sphere_volume(shape)
    lat, faces = _mc(cuda, vol, 10.0)
    world, faces_w = _mc(cuda, vol, 10.0, aabb=aabb)
    assert np.array_equal(faces, faces_w)
    want = mh.lattice_to_world(lat, shape, aabb)
    assert np.array_equal(world.view(np.uint32), want.view(np.uint32))
    # a device tensor works as the box too (model.aabb_infer)
    world_t, _ = _mc(cuda, vol, 10.0, aabb=torch.tensor(aabb, device=cuda))
    assert np.array_equal(world_t, world)


def test_bad_arguments_return_their_codes(cuda):
    """Argument checks only: none of these reaches a kernel (the sentinel in
    counts and the outputs stay as they were)."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    vol = torch.zeros(4, 4, 4, device=cuda)
    ws_bytes = int(lib.ngp_mesh_workspace_bytes(4, 4, 4))
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    counts = torch.full((2,), -7, dtype=torch.int64, device=cuda)
    out = torch.full((8, 3), -7.0, device=cuda)
    faces = torch.full((8, 3), -7, dtype=torch.int32, device=cuda)
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    flipped = (ctypes.c_float * 6)(-1, 1, -1, 1, 1, 1)
    s = nat.stream_of(vol)

    def count(v=P(vol), n=(4, 4, 4), thr=0.5, w=P(ws), wb=ws_bytes, c=P(counts)):
        return lib.ngp_mesh_count(v, n[0], n[1], n[2], thr, w, wb, c, s)

    def emit(v=P(vol), n=(4, 4, 4), thr=0.5, b=box, w=P(ws), wb=ws_bytes, V=8, T=8, o=P(out), f=P(faces)):
        return lib.ngp_mesh_emit(v, n[0], n[1], n[2], thr, b, w, wb, V, T, o, None, f, s)

    def err():
        return lib.ngp_last_error().decode()

    ARG, UNSUPPORTED = -1, -3
    assert count(n=(1, 4, 4)) == ARG and "resolution" in err()
    assert emit(n=(4, 4, 1)) == ARG
    assert lib.ngp_mesh_lattice_points(4, 1, 4, box, 0, 4, P(out), s) == ARG
    # 2^31 points: sizes passed as numbers only, the buffers are the small ones
    assert count(n=(2048, 1024, 1024)) == ARG and "31 bits" in err()
    assert emit(n=(65536, 65536, 2)) == ARG
    assert int(lib.ngp_mesh_workspace_bytes(2048, 1024, 1024)) == 0
    assert int(lib.ngp_mesh_workspace_bytes(1, 4, 4)) == 0
    assert count(v=None) == ARG and "null" in err()
    assert count(c=None) == ARG and count(w=None) == ARG
    assert emit(v=None) == ARG and emit(o=None) == ARG and emit(f=None) == ARG
    assert count(wb=ws_bytes - 1) == ARG and "workspace" in err()
    assert emit(wb=ws_bytes - 1) == ARG
    assert count(thr=float("nan")) == ARG and "finite" in err()
    assert count(thr=float("inf")) == ARG and emit(thr=float("nan")) == ARG
    assert emit(b=flipped) == ARG and "aabb" in err()
    assert lib.ngp_mesh_lattice_points(4, 4, 4, flipped, 0, 4, P(out), s) == ARG
    assert lib.ngp_mesh_lattice_points(4, 4, 4, None, 0, 4, P(out), s) == ARG
    assert lib.ngp_mesh_lattice_points(4, 4, 4, box, 0, 65, P(out), s) == ARG
    assert emit(V=2 ** 31) == UNSUPPORTED and emit(T=2 ** 31) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((out == -7).all()) and bool((faces == -7).all())
    with pytest.raises(RuntimeError, match="float32"):
        from nerf.mesh import marching_cubes
        marching_cubes(vol.double(), 0.5)


# ---- sample_density --------------------------------------------------------------

def _model(cuda, bound=1, seed=0):
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(seed)
    m = NeRFNetwork(bound=bound, cuda_ray=True, density_thresh=10).to(cuda)
    with torch.no_grad():
        m.encoder.embeddings.normal_(0, 0.3)  # densities spread around exp(0) = 1
    return m


def _lattice_np(res, aabb):
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in res], indexing="ij"), -1).reshape(-1, 3)
    return mh.lattice_to_world(idx, res, aabb)


@pytest.fixture(scope="module")
def density24(cuda):
    """(model, its autograd-path density on the 24^3 lattice of aabb_infer)."""
    m = _model(cuda)
    pts = torch.from_numpy(_lattice_np((24, 24, 24), (-1, -1, -1, 1, 1, 1))).to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = m.density(pts)["sigma"].reshape(-1).float()
    return m, pts, ref.cpu().numpy()


def test_lattice_points_match_the_formula(cuda, density24):
    from nerf.mesh import lattice_points
    _, pts, _ = density24
    out = torch.zeros(24 ** 3, 3, device=cuda)
    lattice_points((24, 24, 24), (-1, -1, -1, 1, 1, 1), 0, 24 ** 3, out)
    assert torch.equal(out.view(torch.int32), pts.view(torch.int32))
    part = torch.zeros(100, 3, device=cuda)
    lattice_points((24, 24, 24), (-1, -1, -1, 1, 1, 1), 5000, 5100, part)
    assert torch.equal(part, pts[5000:5100])
    odd = torch.zeros(3 * 5 * 4, 3, device=cuda)
    lattice_points((3, 5, 4), (-1.5, -0.5, 0.25, 2.0, 1.0, 3.0), 0, 60, odd)
    want = _lattice_np((3, 5, 4), (-1.5, -0.5, 0.25, 2.0, 1.0, 3.0))
    assert np.array_equal(odd.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_sample_density_matches_the_autograd_path(cuda, density24):
    from nerf.mesh import sample_density
    m, _, ref = density24
    vol = sample_density(m, 24, chunk=4096)  # 13824 points: three chunks and a ragged fourth
    assert vol.shape == (24, 24, 24) and vol.dtype == torch.float32
    got = vol.reshape(-1).cpu().numpy()
    print(f"sample_density: max rel diff {np.max(np.abs(got - ref) / ref):.3e}, sigma in [{ref.min():.3g}, "
          f"{ref.max():.3g}]")
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    assert torch.equal(sample_density(m, 24, chunk=2 ** 21), vol)


def test_sample_density_covers_aabb_infer(cuda):
    from nerf.mesh import sample_density
    m = _model(cuda, bound=2, seed=1)
    assert m.aabb_infer.tolist() == [-2, -2, -2, 2, 2, 2]
    vol = sample_density(m, 12)
    pts = torch.from_numpy(_lattice_np((12, 12, 12), (-2, -2, -2, 2, 2, 2))).to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = m.density(pts)["sigma"].reshape(-1).float()
    np.testing.assert_allclose(vol.reshape(-1).cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=0)
    assert torch.equal(sample_density(m, 12, aabb=(-2, -2, -2, 2, 2, 2)), vol)
    assert not torch.equal(sample_density(m, 12, aabb=(-1, -1, -1, 1, 1, 1)), vol)


def test_sample_density_fallback_for_other_models(cuda):
    """A model the fused query does not cover (sigma network 32 -> 32) takes
    model.density() under autocast, chunked, on the same lattice."""
    from nerf.mesh import _fused_query, sample_density
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(2)
    m = NeRFNetwork(bound=1, cuda_ray=True, hidden_dim=32).to(cuda)
    with torch.no_grad():
        m.encoder.embeddings.normal_(0, 0.3)
    assert not _fused_query(m)
    vol = sample_density(m, 10, chunk=300)
    pts = torch.from_numpy(_lattice_np((10, 10, 10), (-1, -1, -1, 1, 1, 1))).to(cuda)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = m.density(pts)["sigma"].reshape(-1).float()
    # the same path in chunks of 300 rows: the tolerance the fused query is held to above
    np.testing.assert_allclose(vol.reshape(-1).cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=0)


# ---- end to end ------------------------------------------------------------------

def test_trainer_save_mesh_end_to_end(cuda, tmp_path):
    """~300 fused steps on the three-box scene with the density update on its
    cadence, then FusedTrainer.save_mesh at 64^3."""
    from nerf.fused import FusedTrainer
    from nerf.mesh import read_ply, sample_density
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(cuda)
    model.train()
    data = SyntheticLego(cuda, num_rays=1024)
    model.mark_untrained_grid(data.poses, data.intrinsics)
    ft = FusedTrainer(model, data, M=131072, seed=0)
    with pytest.raises(RuntimeError, match="path is needed"):
        ft.save_mesh()
    for it in range(304):
        if it % 16 == 0:
            ft.update_density()
        ft.step()
    ft.flush()
    vol = sample_density(model, 64)
    thr = 10.0
    if not bool((vol >= 10).any()):  # no sigma >= 10 yet: the median of the positive values
        thr = float(vol[vol > 0].median())
    print(f"end to end: loss {ft.last_loss:.5f}, sigma max {float(vol.max()):.3f}, threshold {thr:g}")
    path, nv, nt = ft.save_mesh(str(tmp_path / "out" / "boxes.ply"), resolution=64, threshold=thr)
    assert os.path.exists(path)
    verts, faces, normals = read_ply(path)
    assert verts.shape == (nv, 3) and faces.shape == (nt, 3) and normals.shape == (nv, 3)
    assert nv > 0 and nt > 0
    box = model.aabb_infer.cpu().numpy()
    assert np.all(verts >= box[:3]) and np.all(verts <= box[3:])
    # the vertex rule against the flushed model's volume
    v = vol.cpu().numpy()
    p, axis, _ = mh.crossed_edges(v, thr)
    want = mh.lattice_to_world(mh.vertex_rule(v, thr, p, axis), v.shape, box)
    assert np.array_equal(verts.view(np.uint32), want.view(np.uint32))
    assert faces.min() >= 0 and faces.max() < nv
    assert np.isfinite(normals).all()
    assert ft.device_errors() == 0
    # the default path: <workspace>/meshes/ngp.ply
    ft.workspace = str(tmp_path / "ws")
    path2, nv2, nt2 = ft.save_mesh(resolution=16, threshold=thr)
    assert path2 == os.path.join(str(tmp_path / "ws"), "meshes", "ngp.ply") and os.path.exists(path2)
    assert read_ply(path2)[0].shape == (nv2, 3)


def _write_scene(path, n, H, W):
    """n RGBA training views of the Lego boxes (and the first as the val split):
    SyntheticLego's analytic target rendered on the CPU, written as PNGs with
    transforms_*.json, as tests/test_gpu_fused_images.py builds its scenes."""
    from PIL import Image

    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n, num_rays=1024)
    frames = []
    for k in range(n):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        img = (rgba.numpy() * 255).round().astype(np.uint8)
        Image.fromarray(img, "RGBA").save(os.path.join(path, f"r_{k}.png"))
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}", "transform_matrix": c2w.tolist()})
    for sp, fr in (("train", frames), ("val", frames[:1])):
        with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)


def test_main_nerf_save_mesh(cuda, tmp_path, capsys):
    import main_nerf
    from nerf.mesh import read_ply
    scene = tmp_path / "scene"
    scene.mkdir()
    _write_scene(str(scene), 6, 32, 32)
    ws = str(tmp_path / "ws")
    out = main_nerf.main([str(scene), "-O", "--workspace", ws, "--bound", "1", "--scale", "1.0", "--dt_gamma", "0",
                          "--num_rays", "1024", "--sample_budget", "131072", "--save_mesh", "--mesh_resolution", "32",
                          "--mesh_threshold", "0.5", "--iters", "32"])
    text = capsys.readouterr().out
    assert out["mesh"] == os.path.join(ws, "meshes", "ngp.ply") and os.path.exists(out["mesh"])
    assert f"{out['mesh_vertices']} vertices, {out['mesh_triangles']} triangles" in text and out["mesh"] in text
    verts, faces, normals = read_ply(out["mesh"])
    assert verts.shape == (out["mesh_vertices"], 3) and faces.shape == (out["mesh_triangles"], 3)
    assert normals.shape == verts.shape
    if len(faces):
        assert faces.min() >= 0 and faces.max() < len(verts)
        assert np.all(np.abs(verts) <= 1.0)
