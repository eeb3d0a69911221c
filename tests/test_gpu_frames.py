"""GPU: finished uint8 frames (nerf/frames.py, csrc/frame.hip) against the
paths they replace: the training draw's rays, get_rays + near_far + render_init,
FusedRenderer.render's blend and depth, the reference-API render, and the
command line's --test round trip.

All at 37 x 53 (frame_helpers): non-square, H * W = 1961 odd, two workgroups
of 1024 pixels with the second one partial and a one-pixel tail."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import frame_helpers as fh
from depth_helpers import write_scene
from frame_helpers import H, W

pytestmark = pytest.mark.gpu

POSE = 7


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def field(cuda):
    """The partly trained Lego field of tests/test_gpu_render.py::_trained,
    trained once for the module: (model in eval mode, data)."""
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(cuda)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(cuda))
    data = SyntheticLego(cuda, num_rays=4096)
    ft = FusedTrainer(model, data, M=200000, seed=1)
    ft.run(150)
    ft.flush()
    torch.cuda.synchronize()
    model.eval()
    return model, data


def _renderer(field, bg_color=1.0, poses=None, capture=True):
    from nerf.frames import FrameRenderer
    model, data = field
    fr = FrameRenderer(model, H, W, fh.scaled_intrinsics(data), bg_color=bg_color)
    fr.load_weights()
    if capture:
        fr.capture()
    fr.set_poses(data.poses[POSE:POSE + 1] if poses is None else poses)
    return fr


def test_rays_are_the_training_rays(cuda, field, parity_report):
    import _ngp_native as nat
    import raymarching
    from nerf.utils import get_rays
    model, data = field
    fr = _renderer(field, capture=False)
    r = fr.renderer
    for t in (r.rays_o, r.rays_d, r.nears, r.fars, r.rays_t, r.noises, r.weights_sum, r.depth, r.image):
        t.fill_(-7.0)  # every element is written by the begin launch
    r.alive[0].fill_(-7)
    r.state.fill_(255)
    fr.begin(0)
    torch.cuda.synchronize()
    N = H * W
    # what ngp_render_init initialises, and zeroed noises
    assert torch.equal(r.alive[0], torch.arange(N, dtype=torch.int32, device=cuda))
    assert torch.equal(_bits(r.rays_t), _bits(r.nears))
    for t in (r.noises, r.weights_sum, r.depth, r.image):
        assert int(_bits(t).abs().max()) == 0
    assert r.state.view(torch.int32).tolist() == [0, N, 0, 0, 0, 0, 0, 0]

    # the training draw (ngp_image_rays) of the single pose: bit-equal at its pixels
    lib, P, n = nat.lib(), nat.ptr, 2048
    f = {k: torch.zeros(n, w, device=cuda) for k, w in (("rays_o", 3), ("rays_d", 3), ("rgba", 4), ("bg", 3))}
    f.update({k: torch.zeros(n, device=cuda) for k in ("nears", "fars", "noises")})
    pix = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    index = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    counter = torch.zeros(2, dtype=torch.int32, device=cuda)
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    pixels = torch.zeros(1, H, W, 4, dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), 65536.0, s), "fused_state_init")
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = P(pixels), 4, nat.DTYPE_U8
    src.pix, src.image_index = P(pix), P(index)
    nat.check(lib.ngp_image_rays(P(fr.poses), 1, fr._intr, H, W, n, ctypes.byref(src), fr._aabb[False],
                                 float(model.min_near), 5, P(state), P(f["rays_o"]), P(f["rays_d"]), P(f["rgba"]),
                                 P(f["bg"]), P(f["nears"]), P(f["fars"]), P(f["noises"]), P(counter), None, s),
              "image_rays")
    torch.cuda.synchronize()
    p = pix.long()
    assert int(p.min()) >= 0 and int(p.max()) < N and p.unique().numel() > N // 4
    for name in ("rays_o", "rays_d", "nears", "fars"):
        assert torch.equal(_bits(f[name]), _bits(getattr(r, name)[p])), name

    # get_rays + near_far on the device
    ref = get_rays(data.poses[POSE:POSE + 1], fh.scaled_intrinsics(data), H, W, -1)
    assert torch.equal(_bits(ref["rays_o"].reshape(N, 3)), _bits(r.rays_o))
    d = float((ref["rays_d"].reshape(N, 3) - r.rays_d).abs().max())
    parity_report(f"{W}x{H}: max |rays_d - get_rays| {d:.3e}")
    assert d <= 1e-6
    nears, fars = raymarching.near_far_from_aabb(r.rays_o, r.rays_d, model.aabb_infer, model.min_near)
    assert torch.equal(_bits(nears), _bits(r.nears)) and torch.equal(_bits(fars), _bits(r.fars))
    assert 0 < int((r.nears > 1e30).sum()) < N  # the view has rays that meet the box and rays that miss it


@pytest.mark.parametrize("bg", [1.0, 0.25])
def test_finish_is_exact(cuda, field, bg):
    fr = _renderer(field, bg_color=bg)
    r = fr.renderer
    rgb8, depth8 = fr.render(0, floats=True)
    torch.cuda.synchronize()
    rgb8, depth8 = rgb8.cpu().numpy(), depth8.cpu().numpy()
    image, depth = fr.image.clone(), fr.depth.clone()
    assert rgb8.shape == (H, W, 3) and depth8.shape == (H, W) and rgb8.dtype == depth8.dtype == np.uint8
    out = r.render(r.rays_o.clone(), r.rays_d.clone(), bg_color=bg)
    torch.cuda.synchronize()
    ws = out["weights_sum"]
    assert float(ws.max()) > 0.5 and float(ws.min()) < 0.5  # opaque and see-through pixels
    assert np.array_equal(fh.q(out["image"].cpu().numpy()).reshape(H, W, 3), rgb8)
    assert np.array_equal(fh.q(out["depth"].cpu().numpy()).reshape(H, W), depth8)
    assert len(np.unique(rgb8)) > 4 and len(np.unique(depth8)) > 4  # a picture, not flat frames
    for got, want in ((image, out["image"]), (depth, out["depth"])):
        fin = torch.isfinite(want)
        assert torch.equal(fin, torch.isfinite(got))
        assert torch.equal(_bits(got)[fin], _bits(want)[fin])


def test_against_the_reference_api_path(cuda, field, parity_report):
    from nerf.utils import get_rays
    model, data = field
    fr = _renderer(field)
    rgb8, depth8 = (t.cpu().numpy() for t in fr.render(0))
    rays = get_rays(data.poses[POSE:POSE + 1], fh.scaled_intrinsics(data), H, W, -1)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = model.render(rays["rays_o"], rays["rays_d"], staged=True, bg_color=1, perturb=False, dt_gamma=0.0,
                           max_steps=1024)
    ref_image = ref["image"].float().reshape(H, W, 3).cpu().numpy()
    ref_depth = ref["depth"].float().reshape(H, W).cpu().numpy()
    dc = np.abs(fh.q(ref_image).astype(np.int32) - rgb8.astype(np.int32))
    fin = np.isfinite(ref_depth)
    dz = np.abs(fh.q(ref_depth).astype(np.int32) - depth8.astype(np.int32))[fin]
    colour, depth = float((dc <= 1).mean()), float((dz <= 1).mean())
    line = (f"{W}x{H}: colour values within one level {colour:.5f} (max {int(dc.max())}), "
            f"depth {depth:.5f} over {int(fin.sum())} finite pixels (max {int(dz.max())})")
    print(line)
    parity_report(line)
    assert fin.sum() > H * W // 2
    assert colour >= 0.999 and depth >= 0.999


def test_all_miss_frame(cuda, field):
    """A camera outside the box looking past it: every pixel is the background, every depth 0 / 0 -> 0."""
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.0, -5.0, 0.0])
    fr = _renderer(field, bg_color=0.25, poses=pose[None])
    rgb8, depth8 = fr.render(0, floats=True)
    torch.cuda.synchronize()
    assert float(fr.renderer.nears.min()) > 1e30  # near = far = FLT_MAX
    assert torch.equal(rgb8, torch.full_like(rgb8, int(fh.q(0.25))))
    assert int(depth8.max()) == 0
    assert torch.isnan(fr.depth).all() and torch.equal(fr.image, torch.full_like(fr.image, 0.25))
    assert fr.renderer.iterations == fr.renderer.K  # the loop ended in its first replay


def test_two_frames_in_sequence(cuda, field):
    model, data = field
    poses = data.poses[[POSE, 31]]
    fr = _renderer(field, poses=poses)
    alone = []
    for k in range(2):
        fr.set_poses(poses[k:k + 1])
        alone.append(tuple(t.cpu().numpy() for t in fr.render(0)))
    assert not np.array_equal(alone[0][0], alone[1][0])
    fr.set_poses(poses)
    assert len(fr) == 2
    for _ in range(2):  # a second pass over the path repeats the first
        g = fr.frames()
        rgb0, depth0 = next(g)
        assert np.array_equal(rgb0, alone[0][0]) and np.array_equal(depth0, alone[0][1])
        rgb1, depth1 = next(g)
        # frame 0's arrays are still frame 0 (the other pinned pair took frame 1)
        assert np.array_equal(rgb0, alone[0][0]) and np.array_equal(depth0, alone[0][1])
        assert np.array_equal(rgb1, alone[1][0]) and np.array_equal(depth1, alone[1][1])
        assert next(g, None) is None


# ---- the command line ----
ARGS = ["-O", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--num_rays", "256", "--sample_budget", "65536"]


def _decode(paths):
    return [np.asarray(Image.open(p)) for p in paths]


def test_main_nerf_test_mode(cuda, tmp_path, capsys):
    import main_nerf
    from nerf.frames import FrameRenderer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import NeRFDataset
    scene = tmp_path / "scene"
    scene.mkdir()
    write_scene(str(scene), 5, 24, 32, heldout=3, depth=False, num_rays=256)
    shutil.copy(scene / "transforms_val.json", scene / "transforms_test.json")
    ws = str(tmp_path / "ws")

    with pytest.raises(SystemExit) as e:  # nothing trained yet
        main_nerf.main([str(scene), *ARGS, "--test", "--workspace", ws])
    assert os.path.join(ws, "checkpoints", "ngp.pth") in str(e.value)

    trained = main_nerf.main([str(scene), *ARGS, "--iters", "32", "--workspace", ws])
    assert "results" not in trained and not os.path.exists(os.path.join(ws, "results"))  # --write_frames is off
    capsys.readouterr()
    out = main_nerf.main([str(scene), *ARGS, "--test", "--workspace", ws])
    text = capsys.readouterr().out
    assert out["frames"] == 3 and "3 frames" in text and "frames/s" in text
    want = [os.path.join(ws, "results", f"ngp_{i:04d}_{kind}.png") for i in range(3) for kind in ("rgb", "depth")]
    assert out["frame_paths"] == want and sorted(os.listdir(os.path.join(ws, "results"))) == \
        sorted(os.path.basename(p) for p in want)

    # the files hold the bytes FrameRenderer gives for the loaded checkpoint
    state = torch.load(trained["checkpoint"], map_location="cpu", weights_only=False)
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=True, density_scale=1, min_near=0.2,
                        density_thresh=10).to(cuda)
    model.load_state_dict(state["model"], strict=False)
    model.eval()
    test = NeRFDataset(str(scene), cuda, type="test", scale=1.0, num_rays=256, store="uint8")
    assert (test.H, test.W) == (24, 32) and test.poses.shape[0] == 3
    fr = FrameRenderer(model, 24, 32, test.intrinsics, dt_gamma=0.0)
    fr.load_weights()
    fr.set_poses(test.poses)
    files = _decode(want)
    for i in range(3):
        rgb8, depth8 = (t.cpu().numpy() for t in fr.render(i))
        assert files[2 * i].shape == (24, 32, 3) and files[2 * i + 1].shape == (24, 32)
        assert np.array_equal(files[2 * i], rgb8) and np.array_equal(files[2 * i + 1], depth8)
    assert len(np.unique(files[0])) > 2  # a picture, not a flat frame


def test_main_nerf_test_mode_interpolates_without_a_test_split(cuda, tmp_path, capsys):
    import main_nerf
    scene = tmp_path / "colmap"
    scene.mkdir()
    write_scene(str(scene), 5, 24, 32, colmap=True, depth=False, num_rays=256)
    assert sorted(p for p in os.listdir(scene) if p.endswith(".json")) == ["transforms.json"]
    ws = str(tmp_path / "ws")
    out = main_nerf.main([str(scene), *ARGS, "--iters", "32", "--workspace", ws, "--write_frames", "--test_frames",
                          "2"])
    assert out["frames"] == 3 and len(os.listdir(os.path.join(ws, "results"))) == 6  # --write_frames after training
    first = _decode(out["frame_paths"])
    shutil.rmtree(os.path.join(ws, "results"))
    out = main_nerf.main([str(scene), *ARGS, "--test", "--workspace", ws, "--test_frames", "3"])
    assert out["frames"] == 4 and "between training views" in capsys.readouterr().out
    assert len(os.listdir(os.path.join(ws, "results"))) == 8
    again = _decode(out["frame_paths"])
    # both paths start and end on the same two training views (--seed): the same end frames
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[-1], again[-1])
    with open(scene / "transforms.json") as f:
        assert len(json.load(f)["frames"]) == 5
