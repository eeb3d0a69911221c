"""CPU: the pieces of image-dataset training that need no GPU: the uint8 image
store of nerf.provider.NeRFDataset against its float32 store, the argument
checks of the C ABI's image entries (ngp_image_source), and main_nerf's
command line. The scene is built here: SyntheticLego's poses, its analytic
target rendered on the CPU, quantised to uint8 and written as PNGs."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image


def _scene(tmp_path, n=3, H=12, W=16):
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n, num_rays=32)
    frames = []
    for k in range(n):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        rgba[..., :3] *= torch.linspace(0.3, 1.0, W)[None, :, None]  # more than the three box colours
        img = (rgba.numpy() * 255).round().astype(np.uint8)
        Image.fromarray(img, "RGBA").save(tmp_path / f"r_{k}.png")
        # the file's pose: SyntheticLego's, which nerf_matrix_to_ngp(scale=1) maps back to itself
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}", "transform_matrix": c2w.tolist()})
    t = {"camera_angle_x": 0.6911112, "frames": frames}
    for sp in ("train", "val"):
        (tmp_path / f"transforms_{sp}.json").write_text(json.dumps(t))
    return lego


def test_uint8_store_equals_float32_store(tmp_path):
    from nerf.provider import NeRFDataset
    lego = _scene(tmp_path)
    cpu = torch.device("cpu")
    f32 = NeRFDataset(str(tmp_path), cpu, scale=1.0, num_rays=32)
    u8 = NeRFDataset(str(tmp_path), cpu, scale=1.0, num_rays=32, store="uint8")
    assert torch.equal(f32.poses, lego.poses)  # the scene's poses are SyntheticLego's
    assert f32.images.dtype == torch.float32 and u8.images.dtype == torch.uint8
    assert u8.images.shape == f32.images.shape == (3, 12, 16, 4)
    assert 0 < int((u8.images[..., 3] > 0).sum()) < u8.images[..., 3].numel()  # the boxes are in view
    assert torch.equal((u8.images.float() / 255).view(torch.int32), f32.images.view(torch.int32))
    for index in (0, 2):
        a = f32.sample(index, torch.Generator().manual_seed(5))
        b = u8.sample(index, torch.Generator().manual_seed(5))
        assert b["images"].dtype == torch.float32
        for key in ("rays_o", "rays_d", "images"):
            assert torch.equal(a[key].contiguous().view(torch.int32), b[key].contiguous().view(torch.int32)), key
    with pytest.raises(ValueError, match="store"):
        NeRFDataset(str(tmp_path), cpu, store="float16")


def _image_entries(lib, src):
    """The three image entries with every other argument empty: the source's
    checks come first and need none of them."""
    s = ctypes.byref(src)
    return [
        ("ngp_image_rays", lambda: lib.ngp_image_rays(
            None, 0, None, 0, 0, 0, s, None, 0.0, 0, *[None] * 11)),
        ("ngp_fused_step_head_images", lambda: lib.ngp_fused_step_head_images(
            None, 0, None, 0, 0, 0, s, None, 0.0, 0, *[None] * 10, 2.0, 0.5, 2000, 1, None, 0, *[None] * 6, 0, None)),
        ("ngp_grid_encode_backward_fused_reduce_batch_images",
         lambda: lib.ngp_grid_encode_backward_fused_reduce_batch_images(
             None, None, 1.0, None, None, 0, None, None, 3, 2, 16, 1.0, 16, 0, 0, 0, None, None, 0, 0, None, 0,
             *[None] * 7, None, s, None)),
    ]


def test_image_entries_reject_bad_sources():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    lib = nat.lib()
    assert lib.ngp_abi_version() == 1 and nat.DTYPE_U8 == 3
    buf = (ctypes.c_uint8 * 64)()  # never read: every case fails its check
    cases = [(dict(channels=5, dtype=nat.DTYPE_U8), "channels"), (dict(channels=2, dtype=0), "channels"),
             (dict(channels=4, dtype=1), "dtype"), (dict(channels=3, dtype=7), "dtype"),
             (dict(channels=4, dtype=nat.DTYPE_U8, pixels=None), "pixels")]
    for fields, word in cases:
        src = nat.ImageSource()
        src.pixels = ctypes.addressof(buf)
        for k, v in fields.items():
            setattr(src, k, v)
        for name, call in _image_entries(lib, src):
            assert call() == -1, (name, fields)  # NGP_ERR_ARG
            msg = lib.ngp_last_error().decode()
            assert word in msg and msg, (name, fields, msg)


def test_main_nerf_command_line(capsys):
    import main_nerf
    with pytest.raises(SystemExit) as e:
        main_nerf.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--bound", "--scale", "--dt_gamma", "--iters", "--num_rays", "--sample_budget", "--workspace"):
        assert flag in out
    p = main_nerf.get_parser()
    d = p.parse_args(["scene"])  # the reference's defaults (main_nerf.py:6-103)
    assert (d.bound, d.scale, d.dt_gamma, d.iters, d.lr, d.num_rays, d.max_steps) == \
        (2, 0.33, 1 / 128, 30000, 1e-2, 4096, 1024)
    assert (d.update_extra_interval, d.density_thresh, d.seed, d.downscale, d.workspace) == (16, 10, 0, 1, "workspace")
    assert d.sample_budget == 2 ** 20
    # the reference's Lego line (readme.md): main_nerf.py data/nerf_synthetic/lego -O --bound 1 --scale 0.8 --dt_gamma 0
    o = p.parse_args(["data/nerf_synthetic/lego", "--workspace", "trial_nerf", "-O", "--bound", "1.0", "--scale",
                      "0.8", "--dt_gamma", "0"])
    assert (o.path, o.workspace, o.bound, o.scale, o.dt_gamma) == ("data/nerf_synthetic/lego", "trial_nerf", 1.0,
                                                                    0.8, 0.0)
