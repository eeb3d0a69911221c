"""The error map on the host side (no GPU): NeRFDataset's map and
nerf.utils.get_rays' error_map branch (the reference's nerf/provider.py:397-401
and nerf/utils.py:101-113, with the map's resolution a parameter)."""
import math

import numpy as np
import pytest
import torch

from depth_helpers import write_scene

H, W, RES, N = 20, 28, 8, 16


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("emap")), 3, 12, 16, depth=False, heldout=1, num_rays=N)


def _dataset(path, **kw):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, torch.device("cpu"), scale=1.0, num_rays=N, **kw)


def test_the_map_is_off_by_default_and_for_other_splits(scene):
    assert _dataset(scene).error_map is None
    assert _dataset(scene, type="val", error_map=True).error_map is None
    assert "inds_coarse" not in _dataset(scene).sample(index=0)


@pytest.mark.parametrize("res", [1, 5, 128])
def test_the_map_is_ones_of_the_right_shape(scene, res):
    data = _dataset(scene, error_map=True, error_map_res=res)
    m = data.error_map
    assert data.error_map_res == res
    assert m.shape == (3, res * res) and m.dtype == torch.float32 and m.is_contiguous()
    assert bool((m == 1).all())


def test_the_default_resolution_is_the_references(scene):
    assert _dataset(scene, error_map=True).error_map.shape == (3, 128 * 128)


@pytest.mark.parametrize("res", [0, -1, 129, 2.5])
def test_a_bad_resolution_raises(scene, res):
    with pytest.raises(ValueError, match="error_map_res"):
        _dataset(scene, error_map=True, error_map_res=res)
    with pytest.raises(ValueError, match="error_map_res"):
        _dataset(scene, error_map_res=res)  # checked whether or not the map is on


def _rays(error_map, seed=0):
    from nerf.utils import get_rays
    g = torch.Generator().manual_seed(seed)
    poses = torch.eye(4)[None]
    return get_rays(poses, np.array([30.0, 30.0, W / 2, H / 2], np.float32), H, W, N, error_map=error_map,
                    generator=g)


def test_get_rays_draws_unique_cells_and_pixels_inside_their_footprints():
    torch.manual_seed(1)
    sx, sy = H / RES, W / RES
    for seed in range(20):
        out = _rays(torch.rand(1, RES * RES) + 0.05, seed)
        cells, inds = out["inds_coarse"][0], out["inds"][0]
        assert out["inds_coarse"].shape == (1, N) and out["inds"].shape == (1, N)
        assert cells.unique().numel() == N and int(cells.min()) >= 0 and int(cells.max()) < RES * RES
        for cell, ind in zip(cells.tolist(), inds.tolist()):
            cx, cy, row, col = cell // RES, cell % RES, ind // W, ind % W
            assert math.floor(cx * sx) <= row <= min(math.ceil((cx + 1) * sx), H - 1), (cell, ind)
            assert math.floor(cy * sy) <= col <= min(math.ceil((cy + 1) * sy), W - 1), (cell, ind)
        # the rays are those pixels' rays
        i, j = (inds % W).float() + 0.5, (inds // W).float() + 0.5
        d = torch.stack(((i - W / 2) / 30.0, (j - H / 2) / 30.0, torch.ones_like(i)), -1)
        assert torch.allclose(out["rays_d"][0], d / d.norm(dim=-1, keepdim=True), atol=1e-6)


def test_get_rays_draws_exactly_the_positive_cells():
    for seed in range(5):
        g = torch.Generator().manual_seed(100 + seed)
        want = torch.randperm(RES * RES, generator=g)[:N]
        w = torch.zeros(1, RES * RES)
        w[0, want] = torch.rand(N, generator=g) + 0.01
        out = _rays(w, seed)
        assert sorted(out["inds_coarse"][0].tolist()) == sorted(want.tolist())


def test_get_rays_rejects_a_map_that_is_no_square():
    with pytest.raises(ValueError, match="error_map"):
        _rays(torch.ones(1, 60))


def test_sample_returns_the_cells_and_the_uniform_draw_is_unchanged(scene):
    """With a map, sample() carries inds_coarse; without one, get_rays draws
    what it drew before the branch existed (the same generator stream)."""
    from nerf.utils import get_rays
    data = _dataset(scene, error_map=True, error_map_res=4)
    out = data.sample(index=1, generator=torch.Generator().manual_seed(0))
    assert out["inds_coarse"].shape == (1, N) and out["inds_coarse"].unique().numel() == N
    poses = torch.eye(4)[None]
    intr = np.array([30.0, 30.0, W / 2, H / 2], np.float32)
    a = get_rays(poses, intr, H, W, N, generator=torch.Generator().manual_seed(5))
    want = torch.randint(0, H * W, size=[N], generator=torch.Generator().manual_seed(5))
    assert torch.equal(a["inds"][0], want) and "inds_coarse" not in a
