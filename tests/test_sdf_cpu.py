"""CPU: the SDF family's references held to independent definitions, and the
host side of sdf/provider.py (prepare_mesh, the file readers). No kernel runs.

The float64 brute-force signed distance of tests/sdf_helpers.py is the
reference of tests/test_gpu_sdf.py; here its sign is held to the generalised
winding number and its value to the analytic box, and the float32 restatement
of the query's arithmetic is held to the bound the GPU test uses."""
import warnings

import numpy as np
import pytest

import sdf  # noqa: F401  (the family under test)
import sdf_helpers as sh
from sdf.provider import prepare_mesh, read_mesh

DIST_BOUND = sh.DIST_BOUND


@pytest.mark.parametrize("name", list(sh.MESHES))
def test_helper_sign_equals_winding_number(name):
    v, f = sh.MESHES[name]()
    assert len(f) == sh.FACES[name]
    pts = sh.make_points(v, f, 900, 1200, seed=3)
    d, _, _ = sh.signed_distance(v, f, pts)
    w = sh.winding_number(v, f, pts)
    use = np.abs(d) >= 1e-9
    assert (~use).sum() <= 0.001 * len(pts)
    inside = w > 0.5
    assert inside[use].sum() > 0 and (~inside[use]).sum() > 0
    assert np.array_equal(d[use] < 0, inside[use]), f"{(~np.equal(d < 0, inside) & use).sum()} mismatches"
    # a closed outward mesh: the winding number is 0 or 1
    assert np.abs(w - np.round(w)).max() < 1e-9


def test_helper_equals_analytic_box():
    v, f = sh.cube()
    pts = sh.make_points(v, f, 1500, 1500, seed=5)
    d, _, _ = sh.signed_distance(v, f, pts)
    assert np.abs(d - sh.box_sdf(pts)).max() <= 1e-12


def _normalised(v):
    vmin, vmax = v.min(0), v.max(0)
    return (v - (vmin + vmax) / 2) * (2 / np.sqrt(np.sum((vmax - vmin) ** 2)) * 0.95)


@pytest.mark.parametrize("name", list(sh.MESHES))
def test_restatement_bound(name):
    """The float32 restatement of the kernel's arithmetic on a prepared
    (normalised) mesh stays within DIST_BOUND / 4 of the float64 reference,
    and few points lie below DIST_BOUND."""
    v, f = sh.MESHES[name]()
    v = _normalised(v)
    pts = sh.query_points(v, f)
    d64, _, _ = sh.signed_distance(v.astype(np.float32), f, pts)  # the float32 corners, as uploaded
    d32, _, _ = sh.signed_distance(v.astype(np.float32), f, pts, dtype=np.float32)
    err = np.abs(d32.astype(np.float64) - d64).max()
    print(f"{name}: max |d32 - d64| = {err:.3e}")
    assert err * 4 <= DIST_BOUND
    far = np.abs(d64) > DIST_BOUND
    assert (~far).mean() <= 0.02
    assert np.array_equal(d32[far] < 0, d64[far] < 0)


def test_prepare_mesh_normalisation_and_layout():
    v, f = sh.torus(32, 16)
    v = v * 3.7 + np.array([5.0, -2.0, 0.25])
    m = prepare_mesh(v, f, device="cpu")
    assert np.allclose(m.vertices, _normalised(v), rtol=0, atol=1e-15)
    assert m.watertight and m.T == 1024
    assert tuple(m.tris.shape) == (1024, 9) and tuple(m.normals.shape) == (1024, 7, 3)
    assert tuple(m.block_aabb.shape) == (16, 6) and tuple(m.cdf.shape) == (1024,)
    tris = m.tris.numpy().reshape(-1, 3, 3)
    assert np.array_equal(tris, m.vertices[m.faces].astype(np.float32))
    # the same faces, reordered
    assert np.array_equal(np.sort(np.sort(m.faces, 1), 0), np.sort(np.sort(f, 1), 0))
    box = m.block_aabb.numpy()
    for k in range(16):
        blk = tris[64 * k:64 * (k + 1)].reshape(-1, 3)
        assert np.array_equal(box[k, :3], blk.min(0)) and np.array_equal(box[k, 3:], blk.max(0))
    cdf = m.cdf.numpy()
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0) and cdf[0] > 0
    # Morton order: a block's box is far smaller than the mesh's
    assert np.median((box[:, 3:] - box[:, :3]).max(1)) < 0.7
    # pseudo-normals: the helper's, in the prepared order
    ref = sh.pseudo_normals(m.vertices, m.faces)
    assert np.abs(m.normals.numpy() - ref).max() < 1e-6


def test_prepare_mesh_partial_block():
    m = prepare_mesh(*sh.bipyramid(), device="cpu")
    assert m.T == 66 and tuple(m.block_aabb.shape) == (2, 6)
    tail = m.tris.numpy()[64:].reshape(-1, 3)
    assert np.array_equal(m.block_aabb.numpy()[1], np.concatenate([tail.min(0), tail.max(0)]))


def test_prepare_mesh_flips_inward_cube(capsys):
    v, f = sh.cube()
    m = prepare_mesh(v, f[:, [0, 2, 1]], device="cpu")
    P = m.vertices[m.faces]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert np.all(np.einsum("ij,ij->i", n, P.mean(1)) > 0)
    assert m.watertight and "not watertight" not in capsys.readouterr().out


def test_prepare_mesh_reports_open_mesh(capsys):
    v, f = sh.cube()
    m = prepare_mesh(v, f[:-1], device="cpu")
    assert not m.watertight
    assert "mesh is not watertight! SDF maybe incorrect." in capsys.readouterr().out


def test_prepare_mesh_drops_degenerate_face_with_warning():
    v, f = sh.cube()
    with pytest.warns(UserWarning, match="dropped 1 zero-area"):
        m = prepare_mesh(v, np.concatenate([f, [[0, 1, 1]]]), device="cpu")
    assert m.T == 12
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        prepare_mesh(v, f, device="cpu")


def test_prepare_mesh_rejects_bad_input():
    v, f = sh.cube()
    bad = f.copy()
    bad[3, 1] = 8
    with pytest.raises(ValueError, match="face index"):
        prepare_mesh(v, bad, device="cpu")
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="face index"):
        prepare_mesh(v, bad, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="no face"):
            prepare_mesh(v, [[0, 0, 1], [2, 2, 2]], device="cpu")


def test_obj_reader_forms(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# a quad and a triangle\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\nv 0 0 1\nf -1 1//1 2/1\nf 1 2 -1\n")
    v, f = read_mesh(str(p))
    assert v.shape == (5, 3) and v.dtype == np.float64
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 4]]


def test_readers_round_trip(tmp_path):
    from nerf.mesh import write_ply
    v, f = sh.icosahedron()
    sh.write_obj(str(tmp_path / "i.obj"), v, f)
    v2, f2 = read_mesh(str(tmp_path / "i.obj"))
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    write_ply(str(tmp_path / "i.ply"), v, f)
    v3, f3 = read_mesh(str(tmp_path / "i.ply"))
    assert np.array_equal(v3, v.astype(np.float32).astype(np.float64)) and np.array_equal(f3, f)
    assert v3.dtype == np.float64 and f3.dtype == np.int64
    with pytest.raises(ValueError):
        read_mesh(str(tmp_path / "i.stl"))


def test_dataset_argument_checks():
    from sdf import SDFDataset, SDFNetwork
    m = prepare_mesh(*sh.cube(), device="cpu")
    with pytest.raises(ValueError, match="divisible by 8"):
        SDFDataset(m, num_samples=12)
    with pytest.raises(RuntimeError, match="CUDA"):
        SDFDataset(m, num_samples=16)
    with pytest.raises(AssertionError):
        SDFNetwork(skips=[2])


def test_sample_rejects_bad_size_before_any_launch():
    import _ngp_native as nat
    rc = nat.lib().ngp_sdf_sample(None, None, 4, 12, 0, None, None, None, None)
    assert rc == -1 and b"divisible by 8" in nat.lib().ngp_last_error()
    assert nat.lib().ngp_sdf_query(None, 0, None, None, None, 4, None, 1, None, None, None) == 0


def test_main_sdf_rejects_tcnn():
    import main_sdf
    with pytest.raises(SystemExit):
        main_sdf.main(["x.obj", "--tcnn"])
