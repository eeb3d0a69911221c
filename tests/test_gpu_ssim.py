"""GPU: SSIM on the device (ngp_frame_ssim in csrc/frame.hip,
nerf.eval.Validator(ssim=True), main_nerf --ssim) against
nerf.eval.ssim_reference, the float64 numpy definition, on the float32 inputs
the squared error compares."""
import contextlib
import ctypes
import io
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch

import ema_helpers as eh
import ssim_helpers as sh

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # NGP_ERR_ARG
MAP_TOL = MEAN_TOL = 1e-10  # both sides in double on identical float32 inputs: summation order alone (<= 2.6e-12)


def _source(nat, pixels):
    src = nat.ImageSource()
    src.pixels, src.channels = nat.ptr(pixels), int(pixels.shape[-1])
    src.dtype = nat.DTYPE_U8 if pixels.dtype == torch.uint8 else nat.DTYPE_CODE[torch.float32]
    return src


def _ssim(H, W, image, ws, bg, pixels, view, out, map_out):
    """ngp_frame_ssim on device tensors -> its return code."""
    import _ngp_native as nat
    src = _source(nat, pixels)
    return nat.lib().ngp_frame_ssim(H, W, nat.ptr(image), nat.ptr(ws), bg, ctypes.byref(src), view, nat.ptr(out),
                                    nat.ptr(map_out), nat.stream_of(out))


@pytest.mark.parametrize("store", sh.STORES)
@pytest.mark.parametrize("H,W", sh.SHAPES, ids=[f"{h}x{w}" for h, w in sh.SHAPES])
def test_entry_against_reference(cuda, parity_report, H, W, store):
    """Map and sum against ssim_reference for both backgrounds and the three
    kinds of input (the cancellation case, noise, smooth)."""
    import _ngp_native as nat
    from nerf.eval import ssim_reference
    count = 3 * (H - 10) * (W - 10)
    worst_map = worst_mean = 0.0
    lowest = 1.0
    for bg in (1.0, 0.25):
        for k, kind in enumerate(sh.KINDS):
            pixels = sh.make_pixels(kind, H, W, store, seed=k)
            assert pixels.shape == (sh.N_VIEWS, H, W, 3 if store == "rgb8" else 4)
            y = sh.ground_truth_np(pixels[sh.VIEW])
            image, ws = sh.make_render(kind, H, W, bg, y, seed=k)
            x = sh.blend_np(image, ws, bg, H, W)
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape == (H, W, 3)
            want_map, want_mean = ssim_reference(x, y)
            out = torch.full((sh.N_VIEWS,), -1.0, dtype=torch.float64, device=cuda)
            got_map = torch.full((count,), -7.0, dtype=torch.float64, device=cuda)
            rc = _ssim(H, W, image.to(cuda), ws.to(cuda), bg, pixels.to(cuda), sh.VIEW, out, got_map)
            assert rc == 0, nat.lib().ngp_last_error()
            torch.cuda.synchronize()
            dm = float(np.abs(got_map.cpu().numpy().reshape(H - 10, W - 10, 3) - want_map).max())
            de = abs(float(out[sh.VIEW]) / count - want_mean)
            print(f"{H}x{W} {store} bg {bg} {kind}: map off by {dm:.3e}, mean {want_mean!r} off by {de:.3e}, "
                  f"lowest value {want_map.min():.4f}")
            worst_map, worst_mean, lowest = max(worst_map, dm), max(worst_mean, de), min(lowest, want_map.min())
            assert dm <= MAP_TOL and de <= MEAN_TOL
            assert out.tolist()[0] == -1.0 and out.tolist()[2] == -1.0
    parity_report(f"{H}x{W} {store}: device SSIM vs float64 numpy, map max abs {worst_map:.3e}, "
                  f"mean max abs {worst_mean:.3e}")
    assert lowest < 0  # the noise inputs reach negative values


def test_identical_images(cuda):
    H, W = 37, 53
    g = torch.Generator().manual_seed(4)
    stack = torch.rand(sh.N_VIEWS, H, W, 3, generator=g).to(cuda)  # float32 RGB: compared as stored
    image = stack[sh.VIEW].reshape(H * W, 3).clone()
    ws = torch.ones(H * W, device=cuda)
    out = torch.zeros(sh.N_VIEWS, dtype=torch.float64, device=cuda)
    for bg in (1.0, 0.25):  # (1 - weights_sum) * bg = 0
        assert _ssim(H, W, image, ws, bg, stack, sh.VIEW, out, None) == 0
        assert abs(float(out[sh.VIEW]) / (3 * (H - 10) * (W - 10)) - 1.0) <= 1e-12


def test_determinism_and_footprint(cuda):
    H, W = 37, 53
    count, guard = 3 * (H - 10) * (W - 10), 64
    pixels = sh.make_pixels("noise", H, W, "rgba8", seed=1)
    y = sh.ground_truth_np(pixels[sh.VIEW])
    image, ws = sh.make_render("smooth", H, W, 1.0, y, seed=1)
    image, ws, pixels = image.to(cuda), ws.to(cuda), pixels.to(cuda)
    runs = []
    for _ in range(2):
        out = torch.full((sh.N_VIEWS,), -1.0, dtype=torch.float64, device=cuda)
        m = torch.full((count + guard,), -7.0, dtype=torch.float64, device=cuda)
        assert _ssim(H, W, image, ws, 1.0, pixels, sh.VIEW, out, m) == 0
        runs.append((out, m))
    (a, ma), (b, mb) = runs
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ma.view(torch.int64),
                                                                                 mb.view(torch.int64))
    assert a.tolist()[0] == -1.0 and a.tolist()[2] == -1.0 and a.tolist()[1] != -1.0
    assert bool((ma[count:] == -7.0).all()) and bool((ma[:count] != -7.0).all())
    c = torch.full((sh.N_VIEWS,), -1.0, dtype=torch.float64, device=cuda)
    assert _ssim(H, W, image, ws, 1.0, pixels, sh.VIEW, c, None) == 0
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))


def test_arguments_and_non_finite(cuda):
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    H, W = 12, 13
    N = H * W
    g = torch.Generator().manual_seed(2)
    image = torch.rand(N + 4, 3, generator=g).to(cuda)
    ws = torch.rand(N + 4, generator=g).to(cuda)
    pixels = torch.randint(0, 256, (2, H, W, 4), generator=g, dtype=torch.uint8).to(cuda)
    out = torch.zeros(2, dtype=torch.float64, device=cuda)
    src = _source(nat, pixels)
    s = nat.stream_of(out)

    def call(h=H, w=W, img=image, wsum=ws, source=src, o=out):
        return lib.ngp_frame_ssim(h, w, P(img), P(wsum), 1.0, None if source is None else ctypes.byref(source), 1,
                                  P(o), None, s)

    assert call() == 0, lib.ngp_last_error()
    assert math.isfinite(float(out[1])) and float(out[0]) == 0.0
    assert call(h=10) == ERR_ARG and b">= 11" in lib.ngp_last_error()
    assert call(w=10) == ERR_ARG and b">= 11" in lib.ngp_last_error()
    assert call(img=image.reshape(-1)[1:]) == ERR_ARG and b"aligned" in lib.ngp_last_error()
    assert call(wsum=ws[1:]) == ERR_ARG and b"aligned" in lib.ngp_last_error()
    assert call(img=None) == ERR_ARG and b"null buffer" in lib.ngp_last_error()
    assert call(wsum=None) == ERR_ARG and b"null buffer" in lib.ngp_last_error()
    assert call(o=None) == ERR_ARG and b"null buffer" in lib.ngp_last_error()
    assert call(source=None) == ERR_ARG and b"null image source" in lib.ngp_last_error()
    bad = _source(nat, pixels)
    bad.channels = 2
    assert call(source=bad) == ERR_ARG and b"2 channels" in lib.ngp_last_error()
    assert call(h=0) == ERR_ARG and b"H * W" in lib.ngp_last_error()
    for value in (float("nan"), float("inf")):
        img = image.clone()
        img[N - 1, 2] = value  # the last pixel
        assert call(img=img) == 0
        assert not math.isfinite(float(out[1]))


def test_validator_ssim(cuda, tmp_path, parity_report):
    from nerf.eval import Validator, ground_truth, ssim_reference
    scene = eh.write_scene(str(tmp_path), 6, 32, 32)
    data = eh.dataset(scene, cuda)
    ft = eh.trainer(cuda, data)
    ft.run(30)
    ft.flush()
    H, W = int(data.H), int(data.W)
    v = Validator(ft.model, data, ssim=True)
    res = v.run()
    assert res["views"] == list(range(6)) and res["ssim"].dtype == np.float64 and res["ssim"].shape == (6,)
    want = []
    for i in range(6):
        v.frames.render(i, floats=True)
        x = v.frames.image.cpu().numpy().reshape(H, W, 3)
        y = ground_truth(data, i).cpu().numpy().reshape(H, W, 3)
        want.append(ssim_reference(x, y)[1])
    off = np.abs(res["ssim"] - np.array(want))
    print(f"validator ssim {res['ssim'].tolist()} off by {off.max():.3e}")
    parity_report(f"32x32, 6 views: Validator ssim vs float64 numpy max abs {off.max():.3e}")
    assert off.max() <= 1e-10
    assert res["mean_ssim"] == float(res["ssim"].mean())
    assert all(-1.0 <= s < 1.0 for s in res["ssim"])
    sub = v.run(views=[2, 0])
    assert sub["views"] == [2, 0] and sub["ssim"].tolist() == [res["ssim"][2], res["ssim"][0]]
    assert sub["mean_ssim"] == float(sub["ssim"].mean())
    plain = Validator(ft.model, data)
    assert plain.ssim is None
    p = plain.run()
    assert "ssim" not in p and "mean_ssim" not in p and sorted(p) == sorted(k for k in res if "ssim" not in k)
    assert p["mse"].tobytes() == res["mse"].tobytes() and p["psnr"].tobytes() == res["psnr"].tobytes()
    assert p["mean_psnr"] == res["mean_psnr"]
    small = types.SimpleNamespace(poses=data.poses, intrinsics=data.intrinsics, H=10, W=32,
                                  images=torch.zeros(6, 10, 32, 4, dtype=torch.uint8, device=cuda), depths=None)
    with pytest.raises(ValueError, match="11"):
        Validator(ft.model, small, ssim=True)


ARGS = ["-O", "--num_rays", "1024", "--sample_budget", "131072", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0"]


def _main(argv):
    """main_nerf.main(argv) -> (its result, what it printed)."""
    import main_nerf
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = main_nerf.main(argv)
    return out, text.getvalue()


def test_main_nerf_ssim(cuda, tmp_path):
    (tmp_path / "scene").mkdir()
    scene = eh.write_scene(str(tmp_path / "scene"), 6, 32, 32, heldout=2)
    shutil.copy(os.path.join(scene, "transforms_val.json"), os.path.join(scene, "transforms_test.json"))
    ws = str(tmp_path / "ws")
    # 18 steps = 3 epochs of 6 views, each validated
    out, text = _main([scene, *ARGS, "--iters", "18", "--workspace", ws, "--eval_interval", "1", "--ssim"])
    assert math.isfinite(out["ssim"]) and -1.0 <= out["ssim"] <= 1.0
    assert len(out["valid_ssim"]) == len(out["valid_psnr"]) == 3
    assert all(math.isfinite(s) and -1.0 <= s <= 1.0 for s in out["valid_ssim"])
    lines = [ln for ln in text.splitlines() if "validation PSNR" in ln]
    assert len(lines) == 3 and all(" SSIM " in ln and ln.rstrip().endswith("s)") for ln in lines), text
    assert f"[main_nerf] SSIM {out['ssim']:.4f} over 2 val images" in text
    final = text.splitlines()
    at = final.index(f"[main_nerf] SSIM {out['ssim']:.4f} over 2 val images")
    assert final[at - 1].startswith("[main_nerf] PSNR ")
    # the last validation saw the weights the final evaluation sees: the same number
    assert out["valid_ssim"][-1] == out["ssim"]

    # --test --ssim: the test split has images
    res, text = _main([scene, *ARGS, "--workspace", ws, "--test", "--ssim"])
    assert math.isfinite(res["psnr"]) and math.isfinite(res["ssim"]) and -1.0 <= res["ssim"] <= 1.0
    assert f"[main_nerf] SSIM {res['ssim']:.4f} over 2 test images" in text
    assert f"[main_nerf] PSNR {res['psnr']:.4f} over 2 test images" in text
    assert res["ssim"] == out["ssim"]  # the test split is the val split here, the weights the checkpoint's
    plain, text = _main([scene, *ARGS, "--workspace", ws, "--test"])
    assert "ssim" not in plain and "psnr" not in plain and "SSIM" not in text

    # without the flag: today's lines and keys
    out2, text2 = _main([scene, *ARGS, "--iters", "18", "--workspace", str(tmp_path / "ws2"), "--eval_interval", "1"])
    assert "SSIM" not in text2 and "ssim" not in out2 and "valid_ssim" not in out2
    assert len(out2["valid_psnr"]) == 3 and sorted(out2) == sorted(k for k in out if "ssim" not in k)
