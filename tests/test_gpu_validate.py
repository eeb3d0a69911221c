"""GPU: the validation pass that stays on the device (ngp_frame_sse in
csrc/frame.hip, nerf.eval.Validator, the `source` of the renderers'
load_weights) against the host path it replaces:
FrameRenderer.render's float image, nerf.eval.ground_truth and nerf.eval.psnr."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import ema_helpers as eh
import frame_helpers as fh

pytestmark = pytest.mark.gpu

ERR_ARG = -1  # NGP_ERR_ARG


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


def _stack(data, cuda, H, W, store, poses=(7, 3, 31)):
    """A dataset of the field's views at H x W: the analytic target of each
    pose as an image stack. store: rgba8 | rgb8 | rgba32 (float32 values that
    are no multiples of 1 / 255)."""
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    intr = fh.scaled_intrinsics(data, H, W)
    lego = SyntheticLego(torch.device("cpu"), num_rays=4096)  # the field's data on the CPU
    assert torch.equal(lego.poses, data.poses.cpu())
    images = []
    for k in poses:
        rays = get_rays(lego.poses[k:k + 1], intr, H, W, -1)
        images.append(lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4).float())
    rgba = torch.stack(images)
    if store == "rgba8":
        img = (rgba * 255).round().to(torch.uint8)
    elif store == "rgb8":
        img = ((rgba[..., :3] * rgba[..., 3:] + (1 - rgba[..., 3:])) * 255).round().to(torch.uint8)
    else:
        g = torch.Generator().manual_seed(5)
        img = (rgba * 0.9 + 0.1 * torch.rand(rgba.shape, generator=g)).float()
    return types.SimpleNamespace(poses=data.poses[list(poses)].contiguous(), intrinsics=intr, H=H, W=W,
                                 images=img.contiguous().to(cuda), depths=None)


def _sse64(c, gt):
    return float(np.sum(((c - gt).astype(np.float32) ** 2).astype(np.float64)))


# 37 x 53: odd N, a tail and a partial second workgroup; 1 x 3: fewer pixels than one thread's run
@pytest.mark.parametrize("store", ["rgba8", "rgb8", "rgba32"])
@pytest.mark.parametrize("H,W", [(fh.H, fh.W), (1, 3)], ids=["37x53", "1x3"])
def test_sse_of_a_rendered_view(cuda, field, parity_report, H, W, store):
    from nerf.eval import Validator, ground_truth
    model, data = field
    stack = _stack(data, cuda, H, W, store)
    assert stack.images.shape == (3, H, W, 3 if store == "rgb8" else 4)
    v = Validator(model, stack)
    v.frames.load_weights()
    view = 1  # not the first image of the stack: the pose's offset into it
    v.frames.render(view, floats=True)
    c = v.frames.image.cpu().numpy()
    gt = ground_truth(stack, view).cpu().numpy()
    assert c.shape == gt.shape == (H * W, 3) and c.dtype == gt.dtype == np.float32
    want = _sse64(c, gt)
    v.sse.fill_(-1.0)
    v.sse_view(view)
    first = v.sse.clone()
    v.sse_view(view)
    torch.cuda.synchronize()
    got = float(v.sse[view])
    rel = abs(got - want) / want
    print(f"{H}x{W} {store}: sse {got!r} numpy {want!r} rel {rel:.3e}")
    parity_report(f"{H}x{W} {store}: device sse vs numpy float64 rel {rel:.3e}")
    assert want > 0 and rel <= 1e-12
    assert torch.equal(first.view(torch.int64), v.sse.view(torch.int64))  # the same from run to run
    assert v.sse.tolist()[0] == -1.0 and v.sse.tolist()[2] == -1.0  # only the view's entry is written


def test_sse_entry_arguments_and_non_finite(cuda):
    """ngp_frame_sse on made-up buffers: its arithmetic against numpy with a
    background other than white, a non-finite colour, and the argument checks."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    H, W = 5, 7
    N = H * W
    g = torch.Generator().manual_seed(2)
    image = torch.rand(N, 3, generator=g).to(cuda)
    ws = torch.rand(N, generator=g).to(cuda)
    pixels = torch.randint(0, 256, (2, H, W, 4), generator=g, dtype=torch.uint8).to(cuda)
    out = torch.zeros(2, dtype=torch.float64, device=cuda)
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = P(pixels), 4, nat.DTYPE_U8
    s = nat.stream_of(out)

    def sse(img, w, bg, pose=1, source=src, o=out):
        return lib.ngp_frame_sse(H, W, P(img), P(w), bg, ctypes.byref(source), pose, P(o), s)

    assert sse(image, ws, 0.25) == 0, lib.ngp_last_error()
    px = pixels[1].reshape(N, 4).cpu().numpy().astype(np.float32) / np.float32(255)
    gt = px[:, :3] * px[:, 3:] + (np.float32(1) - px[:, 3:])
    c = image.cpu().numpy() + ((np.float32(1) - ws.cpu().numpy()) * np.float32(0.25))[:, None]
    want = _sse64(c, gt)
    assert abs(float(out[1]) - want) / want <= 1e-12 and float(out[0]) == 0.0
    for bad in (float("nan"), float("inf")):
        img = image.clone()
        img[N - 1, 2] = bad  # in the tail pixel
        assert sse(img, ws, 1.0) == 0
        assert not math.isfinite(float(out[1]))
    assert sse(image.reshape(-1)[1:], ws, 1.0) == ERR_ARG and b"aligned" in lib.ngp_last_error()
    assert sse(image, ws[1:], 1.0) == ERR_ARG
    assert sse(None, ws, 1.0) == ERR_ARG
    assert lib.ngp_frame_sse(H, W, P(image), P(ws), 1.0, None, 0, P(out), s) == ERR_ARG
    bad = nat.ImageSource()
    bad.pixels, bad.channels, bad.dtype = P(pixels), 2, nat.DTYPE_U8
    assert sse(image, ws, 1.0, source=bad) == ERR_ARG
    assert lib.ngp_frame_sse(0, W, P(image), P(ws), 1.0, ctypes.byref(src), 0, P(out), s) == ERR_ARG


def test_validator_psnr_against_eval_psnr(cuda, field, parity_report):
    """Validator.run against nerf.eval.psnr per view. Both render the pose's
    rays through the same loop; psnr() forms the MSE with torch's float32
    mean. That gap is measured against the float64 sum of the frame
    renderer's own image, and the test allows twice the larger of it and 1e-6."""
    from nerf.eval import Validator, ground_truth, psnr
    model, data = field
    H, W = fh.H, fh.W
    stack = _stack(data, cuda, H, W, "rgba8")
    v = Validator(model, stack)
    res = v.run()
    assert res["views"] == [0, 1, 2] and res["mse"].dtype == np.float64
    gaps = []
    for i in range(3):
        mse_t = 10.0 ** (-psnr(model, stack, i) / 10.0)
        v.frames.render(i, floats=True)
        mse64 = _sse64(v.frames.image.cpu().numpy(), ground_truth(stack, i).cpu().numpy()) / (3 * H * W)
        gap = abs(mse_t - mse64) / mse64
        gaps.append(gap)
        tol = 2 * max(gap, 1e-6)
        got = abs(res["mse"][i] - mse_t) / mse_t
        print(f"view {i}: psnr() mse {mse_t!r}, float64 mse {mse64!r}, gap {gap:.3e}, validator {res['mse'][i]!r}, "
              f"off psnr() by {got:.3e} (allowed {tol:.3e})")
        assert got <= tol
        assert abs(res["psnr"][i] - (-10 * math.log10(mse_t))) <= 10 / math.log(10) * tol * 1.01
        assert abs(res["psnr"][i] + 10.0 * math.log10(res["mse"][i])) <= 1e-12
    parity_report(f"{H}x{W}: psnr()'s float32-mean MSE vs the float64 sum, max relative gap {max(gaps):.3e}")
    # The measured gap sets the tolerance above, so it gets a ceiling of its own: a float32 mean of
    # 3 H W = 5883 squares is good to a few 2^-24 = 6e-8 relative, and the two paths' rays differ in
    # the last bit of rays_d (1.2e-7), which moves single samples; 2.8e-6 was
    # recorded. 1e-5 is under four times that and far below one pixel's share of the MSE (1 / 1961).
    assert max(gaps) <= 1e-5
    assert res["mean_mse"] == float(res["mse"].mean()) and res["mean_psnr"] == float(res["psnr"].mean())
    # a subset, in the order asked for; the model's mode is put back
    model.train()
    sub = v.run(views=[2, 0])
    assert model.training and sub["views"] == [2, 0]
    model.eval()
    assert sub["mse"].tolist() == [res["mse"][2], res["mse"][0]]
    with pytest.raises(IndexError):
        v.run(views=[3])


def test_source_changes_what_is_rendered_and_nothing_else(cuda, tmp_path):
    from nerf.eval import Validator
    from nerf.frames import FrameRenderer
    scene = eh.write_scene(str(tmp_path), 6, 32, 32)
    data = eh.dataset(scene, cuda)
    ft = eh.trainer(cuda, data, ema_decay=0.95)
    ft.run(30)
    ft.flush()
    # other weights into the shadow: the trained ones, perturbed
    g = torch.Generator().manual_seed(9)
    other = [(p.detach().cpu() * 1.5 + 0.01 * torch.randn(p.shape, generator=g)).to(cuda) for p in ft.params]
    for dst, src in zip(ft.ema_params(), other):
        dst.copy_(src)
    holder = eh.model(cuda)  # a model that holds those weights
    with torch.no_grad():
        for p, src in zip([holder.encoder.embeddings, holder.sigma_net.weights, holder.color_net.weights], other):
            p.copy_(src)
    holder.density_bitfield.copy_(ft.model.density_bitfield)
    param, half = ft.flat_param.clone(), ft.flat_half.clone()
    ft.model.eval()
    holder.eval()

    def frame(model, source, capture):
        fr = FrameRenderer(model, data.H, data.W, data.intrinsics)
        fr.load_weights(source)
        if capture:
            fr.capture()
        fr.set_poses(data.poses[:2])
        fr.render(1, floats=True)
        return fr.image.clone(), fr.rgb8.clone(), fr

    own, own8, _ = frame(ft.model, None, True)
    want, want8, _ = frame(holder, None, True)
    got, got8, fr = frame(ft.model, ft.ema_params(), True)
    eager, eager8, _ = frame(ft.model, ft.ema_params(), False)
    assert torch.equal(eh.bits(got), eh.bits(want)) and torch.equal(got8, want8)
    assert torch.equal(eh.bits(eager), eh.bits(want)) and torch.equal(eager8, want8)
    assert not torch.equal(own, want)
    # back to the model's own weights on the same renderer (its graph is captured again)
    fr.load_weights()
    fr.render(1, floats=True)
    assert torch.equal(eh.bits(fr.image), eh.bits(own))
    # the validation pass takes the same source
    v = Validator(ft.model, data)
    a, b = v.run(source=ft.ema_params()), Validator(holder, data).run()
    assert a["mse"].tolist() == b["mse"].tolist() and a["mean_psnr"] == b["mean_psnr"]
    c = v.run()
    assert c["mse"].tolist() == Validator(ft.model, data).run()["mse"].tolist() != a["mse"].tolist()
    with pytest.raises(ValueError, match="source"):
        fr.load_weights(ft.ema_params()[:2])
    torch.cuda.synchronize()
    assert torch.equal(eh.bits(ft.flat_param), eh.bits(param))
    assert torch.equal(ft.flat_half.view(torch.int16), half.view(torch.int16))
    assert ft.model.training is False
