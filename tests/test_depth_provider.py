"""CPU: the depth maps of nerf.provider.NeRFDataset (the reference's dep_path
frames): loading, the nearest resize with the images, the units, sample()'s
gather, and the argument check of the C ABI's image source. The scene is
written by depth_helpers: 3 views at 8 x 12 with depth_k.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

from depth_helpers import write_scene

CPU = torch.device("cpu")


def _stored(path, k):
    with np.load(os.path.join(path, f"depth_{k}.npz")) as f:
        return f["depth"]


@pytest.mark.parametrize("dims", [2, 3])
def test_depths_are_the_files_maps(tmp_path, dims):
    from nerf.provider import NeRFDataset
    path = write_scene(str(tmp_path), 3, 8, 12, depth_dims=dims, num_rays=32)
    assert _stored(path, 0).shape == ((8, 12, 1) if dims == 3 else (8, 12))
    data = NeRFDataset(path, CPU, scale=1.0, num_rays=32)
    assert data.depths.shape == (3, 8, 12) and data.depths.dtype == torch.float32 and data.depths.is_contiguous()
    for k in range(3):
        assert np.array_equal(data.depths[k].numpy(), _stored(path, k).reshape(8, 12))  # file units
    hit = data.depths > 0
    assert 0 < int(hit.sum()) < hit.numel()  # the boxes and the background are both in view
    assert 2.0 < float(data.depths[hit].min()) and float(data.depths.max()) < 4.0  # cameras at radius ~3.2


def test_depth_scale_defaults_to_the_pose_scale(tmp_path):
    from nerf.provider import NeRFDataset
    path = write_scene(str(tmp_path), 3, 8, 12, num_rays=32)
    assert NeRFDataset(path, CPU, scale=0.5, num_rays=32).depth_scale == 0.5
    assert NeRFDataset(path, CPU, scale=0.5, num_rays=32, depth_scale=0.125).depth_scale == 0.125
    a, b = NeRFDataset(path, CPU, scale=0.5, num_rays=32), NeRFDataset(path, CPU, scale=1.0, num_rays=32)
    assert torch.equal(a.depths, b.depths)  # the stack stays in file units


def test_downscale_resizes_depth_with_nearest(tmp_path):
    from nerf.provider import NeRFDataset
    path = write_scene(str(tmp_path), 3, 8, 12, num_rays=32)
    data = NeRFDataset(path, CPU, scale=1.0, num_rays=32, downscale=2)
    assert (data.H, data.W) == (4, 6) and data.images.shape[:3] == (3, 4, 6) and data.depths.shape == (3, 4, 6)
    for k in range(3):
        # cv2.INTER_NEAREST at an integer factor: source index floor(i * 2), no blending of neighbours
        assert np.array_equal(data.depths[k].numpy(), _stored(path, k)[::2, ::2])


def test_sample_gathers_the_batchs_depths(tmp_path):
    from nerf.provider import NeRFDataset
    from nerf.utils import get_rays
    path = write_scene(str(tmp_path), 3, 8, 12, num_rays=32)
    data = NeRFDataset(path, CPU, scale=1.0, num_rays=32, depth_scale=0.3)
    for idx in (0, 2):
        out = data.sample(idx, torch.Generator().manual_seed(7))
        inds = get_rays(data.poses[idx:idx + 1], data.intrinsics, 8, 12, 32,
                        generator=torch.Generator().manual_seed(7))["inds"]
        assert out["depths"].shape == (1, 32) and out["depths"].dtype == torch.float32
        want = data.depths[idx].view(-1)[inds[0]] * data.depth_scale
        assert torch.equal(out["depths"][0].view(torch.int32), want.view(torch.int32))
        assert float(out["depths"].max()) > 0


def test_no_depth_maps_means_none_and_a_partial_set_raises(tmp_path):
    from nerf.provider import NeRFDataset
    os.makedirs(tmp_path / "a")
    plain = write_scene(str(tmp_path / "a"), 3, 8, 12, depth=False, num_rays=32)
    data = NeRFDataset(plain, CPU, scale=1.0, num_rays=32)
    assert data.depths is None and "depths" not in data.sample(0, torch.Generator().manual_seed(1))
    os.makedirs(tmp_path / "b")
    partial = write_scene(str(tmp_path / "b"), 3, 8, 12, no_depth=(1, 2), num_rays=32)
    with pytest.raises(ValueError, match=r"r_1.*dep_path"):  # the first frame without one is named
        NeRFDataset(partial, CPU, scale=1.0, num_rays=32)


def test_image_entries_reject_a_depth_stack_without_its_output():
    """A non-null depth stack with a null output: NGP_ERR_ARG from all three
    image entries, before any device work (every other argument is empty)."""
    import _ngp_native as nat
    from test_image_source import _image_entries
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    lib = nat.lib()
    buf = (ctypes.c_float * 64)()  # never read: the check fails first
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = ctypes.addressof(buf), 4, nat.DTYPE_CODE[torch.float32]
    src.depths, src.depth_scale, src.depth_out = ctypes.addressof(buf), 1.0, None
    for name, call in _image_entries(lib, src):
        assert call() == -1, name
        assert "depth_out" in lib.ngp_last_error().decode(), name


def test_depth_loss_entry_checks_its_job():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    lib = nat.lib()
    loss = (ctypes.c_float * 4)()

    def call(job, loss_ray=ctypes.addressof(loss)):
        return lib.ngp_nerf_composite_loss_depth(None, None, None, None, None, 0, 0, 1e-4, 1.0, None, 4, None, None,
                                                 None, None, None, None, loss_ray,
                                                 ctypes.byref(job) if job is not None else None, None)
    job = nat.DepthLossJob()
    job.color_weight, job.depth_weight = 1.0, 0.5  # a depth weight without the targets
    assert call(job) == -1 and "gt_depth" in lib.ngp_last_error().decode()
    assert call(None) == -1 and "job" in lib.ngp_last_error().decode()
    job.depth_weight = 0.0
    assert call(job, None) == -1 and "loss_ray" in lib.ngp_last_error().decode()
    job.live_cnt = ctypes.addressof(loss)  # one live list of the four
    assert call(job) == -1 and "all or none" in lib.ngp_last_error().decode()
    job.live_cnt = None
    assert call(job) == 0  # N = 0: nothing to do
