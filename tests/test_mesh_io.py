"""CPU: the PLY writer and reader of nerf/mesh.py (numpy only)."""
import numpy as np
import pytest

from nerf.mesh import read_ply, write_ply


def _mesh(seed=0, V=37, T=55):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    v[0, 0] = np.float32(1e-38)  # a denormal-range value and a negative zero survive the round trip
    v[1, 1] = np.float32(-0.0)
    n = rng.standard_normal((V, 3)).astype(np.float32)
    f = rng.integers(0, V, (T, 3)).astype(np.int32)
    return v, f, n


def _header(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii").split("\n")[:-1], data[end:]


@pytest.mark.parametrize("with_normals", [False, True])
def test_round_trip_is_exact(tmp_path, with_normals):
    v, f, n = _mesh()
    path = str(tmp_path / "m.ply")
    write_ply(path, v, f, n if with_normals else None)
    rv, rf, rn = read_ply(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    assert np.array_equal(rv.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(rf, f)
    if with_normals:
        assert np.array_equal(rn.view(np.uint32), n.view(np.uint32))
    else:
        assert rn is None


@pytest.mark.parametrize("with_normals", [False, True])
def test_header_and_payload_size(tmp_path, with_normals):
    v, f, n = _mesh(1, V=5, T=3)
    path = str(tmp_path / "m.ply")
    write_ply(path, v, f, n if with_normals else None)
    lines, payload = _header(path)
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert lines == (["ply", "format binary_little_endian 1.0", "element vertex 5"]
                     + [f"property float {p}" for p in props]
                     + ["element face 3", "property list uchar int vertex_indices", "end_header"])
    assert len(payload) == 5 * 4 * len(props) + 3 * (1 + 3 * 4)
    # the first face record: count 3, then three little-endian int32
    rec = payload[5 * 4 * len(props):][:13]
    assert rec[0] == 3 and np.array_equal(np.frombuffer(rec[1:], "<i4"), f[0])


def test_empty_mesh_is_a_valid_file(tmp_path):
    path = str(tmp_path / "empty.ply")
    write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    lines, payload = _header(path)
    assert "element vertex 0" in lines and "element face 0" in lines and payload == b""
    v, f, n = read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
