"""GPU: the fused engine trained on image datasets (the device-side pixel
gather: ngp_image_source, the image forms of the draw entries, nerf.eval and
main_nerf).

The scenes are built here: SyntheticLego's poses, its analytic target rendered
on the CPU through get_rays, quantised to uint8 and written as PNGs with a
transforms*.json, then loaded by nerf.provider.NeRFDataset like any scene."""
import copy
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from PIL import Image

pytestmark = pytest.mark.gpu

N_RAYS = 1024
M_ROWS = 30000 + 128 - 30000 % 128  # 30000 rounded up to a multiple of 128


def _write_scene(path, n, H, W, channels=4, colmap=False, heldout=0):
    """n training views (+ `heldout` more as the val split) of the Lego boxes.
    colmap: one transforms.json with fx != fy and an off-centre principal point."""
    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n + heldout, num_rays=N_RAYS)
    intr = np.array([1.9 * W, 2.3 * H, 0.46 * W, 0.55 * H], np.float32) if colmap else lego.intrinsics
    frames = []
    for k in range(n + heldout):
        rays = get_rays(lego.poses[k:k + 1], intr, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        if channels == 3:  # RGB files show the solid on white
            rgba = rgba[..., :3] * rgba[..., 3:] + (1 - rgba[..., 3:])
        img = (rgba.numpy() * 255).round().astype(np.uint8)
        Image.fromarray(img, "RGBA" if channels == 4 else "RGB").save(os.path.join(path, f"r_{k}.png"))
        # the file's pose: the one nerf_matrix_to_ngp(scale=1) maps to SyntheticLego's
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}" + (".png" if colmap else ""), "transform_matrix": c2w.tolist()})
    if colmap:
        t = {"fl_x": float(intr[0]), "fl_y": float(intr[1]), "cx": float(intr[2]), "cy": float(intr[3]), "h": H,
             "w": W, "frames": frames}
        with open(os.path.join(path, "transforms.json"), "w") as f:
            json.dump(t, f)
    else:
        for sp, fr in (("train", frames[:n]), ("val", frames[n:] or frames[:1])):
            with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
                json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """The module's scenes, written once."""
    def make(name, *args, **kw):
        return _write_scene(str(tmp_path_factory.mktemp(name)), *args, **kw)
    return {"colmap": make("colmap", 5, 24, 40, colmap=True),
            "lego32": make("lego32", 6, 32, 32),
            "rgb32": make("rgb32", 6, 32, 32, channels=3),
            "lego64": make("lego64", 8, 64, 64, heldout=1)}


def _dataset(path, dev, store="uint8", type="train"):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, dev, type=type, scale=1.0, num_rays=N_RAYS, store=store)


def _model(dev):
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    with torch.no_grad():  # a non-trivial field: larger table values than the 1e-4 init
        model.encoder.embeddings.normal_(0, 0.05)
    model.density_bitfield.copy_(torch.from_numpy(lego_bitfield()).to(dev))
    return model


def _trainer(dev, data, seed=3, options=None, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(_model(dev), data, M=M_ROWS, seed=seed, options=options, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_gather(cuda, scenes):
    """Ray n's target is its pixel of the drawn image, its ray that pixel's
    get_rays ray (fx != fy, off-centre principal point, H != W)."""
    import raymarching
    from nerf.utils import get_rays
    data = _dataset(scenes["colmap"], cuda)
    f32 = _dataset(scenes["colmap"], cuda, store="float32")
    H, W = data.H, data.W
    assert (H, W) == (24, 40) and data.images.shape == (5, 24, 40, 4) and data.images.dtype == torch.uint8
    assert data.intrinsics[0] != data.intrinsics[1] and data.intrinsics[2] != W / 2
    ft = _trainer(cuda, data)
    assert ft._src is not None
    ft._sample()
    torch.cuda.synchronize()
    pix, idx = ft.pix.long(), int(ft.image_index)
    assert int(pix.min()) >= 0 and int(pix.max()) < H * W and pix.unique().numel() > N_RAYS // 4
    assert 0 <= idx < 5
    want = f32.images[idx].view(-1, 4)[pix]  # np.float32(v) / 255 of the same PNGs
    assert torch.equal(_bits(ft.rgba), _bits(want))
    assert 0.02 < float(ft.rgba[:, 3].mean()) < 0.98  # boxes and background both drawn
    assert torch.equal(ft.rays_o, data.poses[idx, :3, 3].expand_as(ft.rays_o))
    rays = get_rays(data.poses[idx:idx + 1], data.intrinsics, H, W, -1)
    assert torch.allclose(ft.rays_d, rays["rays_d"][0][pix], atol=1e-6)
    nears, fars = raymarching.near_far_from_aabb(ft.rays_o, ft.rays_d, ft.model.aabb_train, ft.model.min_near)
    assert torch.equal(_bits(nears), _bits(ft.nears)) and torch.equal(_bits(fars), _bits(ft.fars))
    assert 0.0 <= float(ft.bg.min()) and float(ft.bg.max()) < 1.0  # RGBA: a random background
    assert int(ft.counter.abs().sum()) == 0
    # a new step draws a new batch (the sampler bumps its own draw counter)
    p0, d0 = ft.pix.clone(), int(ft._state_i()[9])
    ft._sample()
    assert int(ft._state_i()[9]) == d0 + 1
    assert not torch.equal(p0, ft.pix)


def test_same_streams_as_the_analytic_draw(cuda, scenes):
    """Same seed, poses and intrinsics: everything but the target is the
    analytic draw's, bit for bit, and the target is its quantised pixel."""
    from nerf.provider import SyntheticLego
    data = _dataset(scenes["lego32"], cuda)
    lego = SyntheticLego(cuda, H=32, W=32, n_poses=6, num_rays=N_RAYS)
    assert torch.equal(data.poses, lego.poses) and np.array_equal(data.intrinsics, lego.intrinsics)
    a, b = _trainer(cuda, data), _trainer(cuda, lego)
    assert a._src is not None and b._src is None
    for draw in range(2):
        a._sample()
        b._sample()
        torch.cuda.synchronize()
        for name in ("rays_o", "rays_d", "bg", "noises", "nears", "fars"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (draw, name)
        # the images are the analytic target rounded to 1/255
        assert float((a.rgba - b.rgba).abs().max()) <= 0.5 / 255 + 1e-6
        assert float(a.rgba[:, 3].mean()) > 0.02


def test_uint8_and_float32_stores_draw_the_same_targets(cuda, scenes):
    a = _trainer(cuda, _dataset(scenes["colmap"], cuda, store="uint8"))
    b = _trainer(cuda, _dataset(scenes["colmap"], cuda, store="float32"))
    assert a._images.dtype == torch.uint8 and b._images.dtype == torch.float32
    for _ in range(2):
        a._sample()
        b._sample()
        torch.cuda.synchronize()
        assert torch.equal(a.pix, b.pix) and torch.equal(a.image_index, b.image_index)
        assert torch.equal(_bits(a.rgba), _bits(b.rgba))


def test_image_rays_entry_draws_the_step_heads_batch(cuda, scenes):
    """ngp_image_rays on its own buffers and a fresh state: draw 0 of the same
    seed, the batch FusedTrainer._sample() (ngp_fused_step_head_images) draws."""
    import ctypes

    import _ngp_native as nat
    data = _dataset(scenes["colmap"], cuda)
    ft = _trainer(cuda, data)
    ft._sample()
    lib, P, N = nat.lib(), nat.ptr, N_RAYS
    f = {k: torch.zeros(N, w, device=cuda) for k, w in (("rays_o", 3), ("rays_d", 3), ("rgba", 4), ("bg", 3))}
    f.update({k: torch.zeros(N, device=cuda) for k in ("nears", "fars", "noises")})
    pix, index = torch.full((N,), -1, dtype=torch.int32, device=cuda), torch.full((1,), -1, dtype=torch.int32,
                                                                                 device=cuda)
    counter = torch.full((2,), 7, dtype=torch.int32, device=cuda)
    state = torch.zeros(lib.ngp_fused_state_bytes(), dtype=torch.uint8, device=cuda)
    s = nat.stream_of(state)
    nat.check(lib.ngp_fused_state_init(P(state), 65536.0, s), "fused_state_init")
    src = nat.ImageSource()
    src.pixels, src.channels, src.dtype = P(data.images), 4, nat.DTYPE_U8
    src.pix, src.image_index = P(pix), P(index)
    nat.check(lib.ngp_image_rays(P(data.poses), data.poses.shape[0], ft._intr, data.H, data.W, N, ctypes.byref(src),
                                 ft._aabb, float(ft.model.min_near), ft.seed, P(state), P(f["rays_o"]),
                                 P(f["rays_d"]), P(f["rgba"]), P(f["bg"]), P(f["nears"]), P(f["fars"]),
                                 P(f["noises"]), P(counter), None, s), "image_rays")
    torch.cuda.synchronize()
    for name, t in f.items():
        assert torch.equal(_bits(t), _bits(getattr(ft, name))), name
    assert torch.equal(pix, ft.pix) and torch.equal(index, ft.image_index)
    assert int(state.view(torch.int32)[9]) == 1 and int(counter.abs().sum()) == 0  # draw counted, counter reset


def test_options_without_an_image_draw_raise(cuda, scenes):
    """march_adam=False draws in ngp_fused_optimizer_update_head, which has no
    image form: a ValueError naming the option, never a silent boxes draw.
    With split_head=True as well the head launch draws, from the images."""
    data = _dataset(scenes["lego32"], cuda)
    with pytest.raises(ValueError, match="march_adam"):
        _trainer(cuda, data, options=dict(march_adam=False))
    a = _trainer(cuda, data, options=dict(march_adam=False, split_head=True))
    b = _trainer(cuda, data, options=dict(draw_ahead=False))
    assert a._src is not None and not a._merge_head and not a._march_adam and not a._draw_ahead
    f32 = _dataset(scenes["lego32"], cuda, store="float32")
    for i in range(3):
        a.step()
        b.step()
        torch.cuda.synchronize()
        want = f32.images[int(a.image_index)].view(-1, 4)[a.pix.long()]
        assert torch.equal(_bits(a.rgba), _bits(want)), i
        assert torch.equal(a.pix, b.pix) and torch.equal(_bits(a.rgba), _bits(b.rgba)), i
        assert a.sample_count() == b.sample_count() > 0, i
    assert np.isfinite(a.last_loss)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


@pytest.mark.parametrize("store", ["uint8", "float32"])
def test_rgb_images_train_on_white(cuda, scenes, store):
    """3-channel images: alpha 1 on a white background (the reference's
    bg_color = 1), and the step equals the autograd step with bg_color=1,
    gt=images (test_fused_forward_backward_matches_autograd's tolerances)."""
    data = _dataset(scenes["rgb32"], cuda, store=store)
    f32 = _dataset(scenes["rgb32"], cuda, store="float32")
    assert data.images.shape == (6, 32, 32, 3)
    from nerf.fused import FusedTrainer
    model = _model(cuda)
    ref = copy.deepcopy(model)
    ref.mean_count = 30000
    ft = FusedTrainer(model, data, M=M_ROWS, seed=3)
    ft._sample()
    torch.cuda.synchronize()
    gt = f32.images[int(ft.image_index)].view(-1, 3)[ft.pix.long()]
    assert torch.equal(_bits(ft.rgba[:, :3]), _bits(gt))
    assert bool((ft.rgba[:, 3] == 1).all()) and bool((ft.bg == 1).all())
    assert float(gt.min()) < 0.9  # not only background
    ft.noises.zero_()  # the autograd call below marches with perturb=False
    ft._forward_backward()
    torch.cuda.synchronize()
    scale = ft.scale
    ref.train()
    with torch.autocast("cuda", dtype=torch.float16):
        out = ref.render(ft.rays_o.clone()[None], ft.rays_d.clone()[None], staged=False, bg_color=1, perturb=False,
                         force_all_rays=False, dt_gamma=0.0, max_steps=1024)
        loss = ((out["image"][0] - gt) ** 2).mean(-1).mean()
    (loss * scale).backward()
    torch.cuda.synchronize()
    assert int(ft.counter[0]) == int(ref.step_counter[0, 0]) > 0
    fused_loss = float(ft.loss_ray.double().sum()) / ft.N
    lv = float(loss.detach())
    print(f"rgb {store}: samples {int(ft.counter[0])} loss fused {fused_loss:.8f} autograd {lv:.8f}")
    assert abs(fused_loss - lv) <= 1e-3 * abs(lv) + 1e-7
    refs = [ref.encoder.embeddings.grad, ref.sigma_net.weights.grad, ref.color_net.weights.grad]
    for name, g, r in zip(["embeddings", "sigma_net", "color_net"], ft.grads, refs):
        print(f"rgb {store}: grad {name} rel {_rel(g, r):.3e}")
        assert torch.isfinite(g.float()).all(), name
        assert r.abs().max() > 0, name
        assert _rel(g, r) < 1e-2, (name, _rel(g, r))


@pytest.mark.parametrize("live", [True, False])
def test_both_draw_sites_draw_the_same_batches(cuda, scenes, live):
    """The draw in the grid backward's bin launch (draw_ahead, the default;
    over the live rows or all rows) against the draw in the head launch
    (draw_ahead=False). After step i the draw-ahead trainer's buffers hold
    batch i + 1 and the other's batch i, so a's batch after step i is compared
    with b's after step i + 1; the sample count and the loss are step i's."""
    data = _dataset(scenes["lego32"], cuda)
    a = _trainer(cuda, data, options=dict(live_rows=live))
    b = _trainer(cuda, data, options=dict(live_rows=live, draw_ahead=False))
    assert a._draw_ahead and a._live == live and not b._draw_ahead
    batches = []
    for i in range(4):
        if i < 3:
            a.step()
        b.step()
        torch.cuda.synchronize()
        if i > 0:  # b holds batch i, which a drew during step i - 1
            pa, ra, ia = batches[i - 1]
            assert torch.equal(pa, b.pix) and torch.equal(ia, b.image_index), i
            assert torch.equal(_bits(ra), _bits(b.rgba)), i
        if i < 3:
            assert a._ahead
            batches.append((a.pix.clone(), a.rgba.clone(), a.image_index.clone()))
            ca, cb = a.sample_count(), b.sample_count()
            la, lb = a.last_loss, b.last_loss
            print(f"live={live} step {i}: samples {ca} / {cb}, loss {la!r} / {lb!r}")
            assert ca == cb > 0, i
            assert la == lb and np.isfinite(la), (i, la, lb)


def _heldout_mse(model, val):
    from nerf.eval import psnr
    return 10.0 ** (-psnr(model, val, 0) / 10.0)


def test_training_on_images_learns_the_scene(cuda, scenes):
    """8 RGBA views at 64 x 64: the loss falls, and so does the error on a 9th
    view the training never saw."""
    data = _dataset(scenes["lego64"], cuda)
    val = _dataset(scenes["lego64"], cuda, type="val")
    assert data.images.shape == (8, 64, 64, 4) and val.images.shape == (1, 64, 64, 4)
    assert not any(torch.equal(val.poses[0], p) for p in data.poses)
    ft = _trainer(cuda, data)
    mse0 = _heldout_mse(ft.model, val)
    for _ in range(4):
        ft.step()
    first = ft.last_loss
    ft.capture()
    ft.run(200)
    late = ft.last_loss
    torch.cuda.synchronize()
    mse1 = _heldout_mse(ft.model, val)
    print(f"loss {first:.6f} -> {late:.6f}; held-out mse {mse0:.6f} -> {mse1:.6f}")
    assert np.isfinite(late) and late < first
    assert ft.device_errors() == 0
    assert np.isfinite(mse1) and mse1 < mse0


def test_main_nerf_trains_evaluates_and_saves(cuda, scenes, tmp_path, capsys):
    import main_nerf
    from nerf.fused import FusedTrainer
    ws = str(tmp_path / "ws")
    out = main_nerf.main([scenes["lego64"], "-O", "--workspace", ws, "--bound", "1", "--scale", "1.0", "--dt_gamma",
                          "0", "--iters", "64", "--num_rays", "1024", "--sample_budget", "131072"])
    text = capsys.readouterr().out
    assert "PSNR" in text and "sample budget" in text and "loss" in text
    assert np.isfinite(out["psnr"]) and np.isfinite(out["loss"])
    assert os.path.exists(out["checkpoint"])
    state = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert state["global_step"] == 64
    ft = FusedTrainer(_model(cuda), _dataset(scenes["lego64"], cuda), M=M_ROWS)
    ft.load_checkpoint(state)
    assert 0 < ft.optimizer_steps <= 64  # (GradScaler may skip the first steps at its initial scale)
    for p, (k, v) in zip(ft.params, [(k, state["model"][k]) for k in
                                     ("encoder.embeddings", "sigma_net.weights", "color_net.weights")]):
        assert torch.equal(p.detach().cpu(), v), k


# ---- data parallel: two ranks on the one GPU (gloo), as tests/test_gpu_fused_dp.py ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, path, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "torch-ngp_amd")]
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ft = _trainer(dev, _dataset(path, dev), seed=0, distributed=True)
    assert ft.dp and ft._draw_ahead and ft._live and ft._src is not None
    pix = []
    for _ in range(3):
        ft.step()
        torch.cuda.synchronize()
        pix.append((int(ft.image_index), ft.pix.cpu().numpy()))
    ft.capture(warmup=1)
    for _ in range(2):
        ft.step()
    ft.flush()
    torch.cuda.synchronize()
    q.put((rank, [p.detach().cpu().numpy() for p in ft.params], pix, ft.optimizer_steps, ft.last_loss))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_ranks_draw_their_own_pixels(scenes):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, scenes["lego32"], q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, p0, x0, s0, l0), (_, p1, x1, s1, l1) = out
    assert s0 == s1 >= 5 and np.isfinite(l0) and np.isfinite(l1)
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)
    for (i0, a), (i1, b) in zip(x0, x1):
        assert 0 <= a.min() and a.max() < 32 * 32 and 0 <= i0 < 6 and 0 <= i1 < 6
        assert not np.array_equal(a, b)
