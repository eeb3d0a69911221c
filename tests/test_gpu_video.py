"""GPU: the test render as Motion-JPEG (nerf.frames.write_video, the command
line's --video): the frames in the .avi files are JpegEncoder's encodings of
the frames FrameRenderer renders, the PNGs beside them are write_frames', and
without the flags a run writes what it wrote before.

A small field (40 steps on the Lego bitfield) at 16 x 24, three poses."""
import os
import shutil

import numpy as np
import pytest
import torch

import frame_helpers as fh
import jpeg_helpers as jh
from depth_helpers import write_scene

pytestmark = pytest.mark.gpu

H, W = 16, 24
POSES = [7, 19, 31]


@pytest.fixture(scope="module")
def renderer(cuda):
    from nerf.frames import FrameRenderer
    from nerf.fused import FusedTrainer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego, lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(cuda)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(cuda))
    data = SyntheticLego(cuda, num_rays=1024)
    ft = FusedTrainer(model, data, M=60000, seed=1)
    ft.run(40)
    ft.flush()
    torch.cuda.synchronize()
    model.eval()
    fr = FrameRenderer(model, H, W, fh.scaled_intrinsics(data, H, W))
    fr.load_weights()
    fr.capture()
    fr.set_poses(data.poses[POSES])
    return fr


def _expected(renderer, quality):
    from nerf.jpeg import JpegEncoder
    rgb, depth = JpegEncoder(H, W, 3, quality, renderer.dev), JpegEncoder(H, W, 1, quality, renderer.dev)
    out = []
    for i in range(len(renderer)):
        rgb8, depth8 = renderer.render(i)
        out.append((rgb.encode(rgb8), depth.encode(depth8), rgb8.cpu().numpy(), depth8.cpu().numpy()))
    return out


@pytest.mark.parametrize("png", [True, False])
def test_write_video(cuda, renderer, tmp_path, png):
    from nerf.frames import write_frames, write_video
    from nerf.video import read_avi
    out = str(tmp_path / "v")
    videos, paths = write_video(renderer, out, "ngp", fps=25, quality=90, png=png)
    assert videos == [os.path.join(out, "ngp_rgb.avi"), os.path.join(out, "ngp_depth.avi")]
    want = _expected(renderer, 90)
    assert len({w[0] for w in want}) == 3  # three different pictures
    for k, (path, mode) in enumerate(zip(videos, ("RGB", "L"))):
        info, frames = read_avi(path)
        assert (info["frames"], info["width"], info["height"], info["fps"], info["handler"]) == (3, W, H, 25, "MJPG")
        assert len(frames) == 3
        for i, f in enumerate(frames):
            assert f == want[i][k], (path, i)
            im = jh.pil_decode(f)
            assert im.mode == mode and im.size == (W, H)
            # ... and it is the frame. At quality 90 no quantiser is above 20, so a coefficient is off by at
            # most 10 and, were every one of them uniformly off, a pixel of R or B (Y + 1.402 Cr, Y + 1.772 Cb)
            # by 9 to 11 levels rms; a mean absolute difference of 12 is above anything the encoder may do and
            # far below another frame's or a scrambled one's
            assert np.abs(np.asarray(im).astype(np.int32) - want[i][2 + k].astype(np.int32)).mean() < 12
    if png:
        ref_dir = str(tmp_path / "f")
        ref = write_frames(renderer, ref_dir, "ngp")
        assert [os.path.basename(p) for p in paths] == [os.path.basename(p) for p in ref] and len(ref) == 6
        for a, b in zip(paths, ref):
            assert open(a, "rb").read() == open(b, "rb").read(), a
        assert sorted(os.listdir(out)) == sorted([os.path.basename(p) for p in ref] +
                                                 ["ngp_rgb.avi", "ngp_depth.avi"])
    else:
        assert paths == [] and sorted(os.listdir(out)) == ["ngp_depth.avi", "ngp_rgb.avi"]


def test_write_video_quality_and_fps(cuda, renderer, tmp_path):
    from nerf.frames import write_video
    from nerf.video import read_avi
    videos, _ = write_video(renderer, str(tmp_path), "low", fps=10, quality=30, png=False)
    want = _expected(renderer, 30)
    info, frames = read_avi(videos[0])
    assert info["fps"] == 10 and info["usec_per_frame"] == 100000
    assert frames == [w[0] for w in want]
    assert sum(map(len, frames)) < sum(len(w[0]) for w in _expected(renderer, 90))


ARGS = ["-O", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--num_rays", "256", "--sample_budget", "65536"]


def test_main_nerf_video_flags(cuda, tmp_path, capsys):
    import main_nerf
    from nerf.video import read_avi
    scene = tmp_path / "scene"
    scene.mkdir()
    write_scene(str(scene), 5, 24, 32, heldout=3, depth=False, num_rays=256)
    shutil.copy(scene / "transforms_val.json", scene / "transforms_test.json")
    ws = str(tmp_path / "ws")
    results = os.path.join(ws, "results")
    main_nerf.main([str(scene), *ARGS, "--iters", "32", "--workspace", ws])

    plain = main_nerf.main([str(scene), *ARGS, "--test", "--workspace", ws])
    assert "video_paths" not in plain
    pngs = sorted(os.listdir(results))
    assert len(pngs) == 6 and all(p.endswith(".png") for p in pngs)
    png_bytes = {p: open(os.path.join(results, p), "rb").read() for p in pngs}
    shutil.rmtree(results)

    capsys.readouterr()
    out = main_nerf.main([str(scene), *ARGS, "--test", "--video", "--workspace", ws])
    assert "ngp_rgb.avi" in capsys.readouterr().out
    assert out["video_paths"] == [os.path.join(results, "ngp_rgb.avi"), os.path.join(results, "ngp_depth.avi")]
    assert sorted(os.listdir(results)) == sorted(pngs + ["ngp_rgb.avi", "ngp_depth.avi"])
    assert {p: open(os.path.join(results, p), "rb").read() for p in pngs} == png_bytes
    assert out["frames"] == 3 and len(out["frame_paths"]) == 6
    for path, mode, shape in zip(out["video_paths"], ("RGB", "L"), ((24, 32, 3), (24, 32))):
        info, frames = read_avi(path)
        assert (info["frames"], info["width"], info["height"], info["fps"]) == (3, 32, 24, 25)
        for i, f in enumerate(frames):
            im = jh.pil_decode(f)
            assert im.mode == mode and np.asarray(im).shape == shape
            kind = "rgb" if mode == "RGB" else "depth"
            png = np.asarray(jh.pil_decode(png_bytes[f"ngp_{i:04d}_{kind}.png"])).astype(np.int32)
            assert np.abs(np.asarray(im).astype(np.int32) - png).mean() < 12  # as in test_write_video
    shutil.rmtree(results)

    out = main_nerf.main([str(scene), *ARGS, "--test", "--video_only", "--video_fps", "12", "--video_quality", "50",
                          "--workspace", ws])
    assert sorted(os.listdir(results)) == ["ngp_depth.avi", "ngp_rgb.avi"] and out["frame_paths"] == []
    assert read_avi(out["video_paths"][0])[0]["fps"] == 12
    with pytest.raises(SystemExit):
        main_nerf.main([str(scene), *ARGS, "--test", "--video", "--video_quality", "0", "--workspace", ws])
