"""Train a scene on the fused engine: `python main_nerf.py <scene> -O`.

The reference's entry point (main_nerf.py:6-103, 105-230) for the instant-ngp
configuration (-O: fp16, cuda_ray, preloaded images), with its flag names and
defaults, on nerf.fused.FusedTrainer: the images stay on the device as uint8
and every batch is gathered there (the engine's image source), the steps
between two density-grid updates replay as captured graphs, and nothing syncs
with the host per step. --save_mesh writes the trained density field's
triangle mesh (device marching cubes, nerf/mesh.py) to
<workspace>/meshes/ngp.ply after the evaluation, where the reference calls
trainer.save_mesh (main_nerf.py:190 / :241). --depth_loss_weight > 0 adds the
reference's depth supervision on scenes whose frames carry a dep_path: the
loss is color_loss_weight * rgb + depth_loss_weight * dep (nerf/utils.py
:545-553, 951-954), the depths gathered on the device beside the colours.
--dist_loss_weight W > 0 adds W times the mean over a
batch's rays of the distortion regulariser (the reference's loss.py
EffDistLoss on the composite's own weights), formed
inside the composite launch; the log line then carries `dist`, and the eval
split's mean ray distortion is printed after the PSNR.
--error_map is the reference's importance sampling (nerf/utils.py:101-113,
578-600): a coarse error image per training view (--error_map_res cells a
side, the reference's 128), the batch's pixels drawn from it without
replacement on the device, each ray's colour error folded back into it.
--test trains nothing: it loads <workspace>/checkpoints/ngp.pth (--ckpt),
renders the test split's poses, or --test_frames steps between two training
poses where the scene has no transforms_test.json, and writes
<workspace>/results/ngp_<i>_rgb.png and _depth.png, as the reference's
trainer.test does (main_nerf.py:188 / :239); --write_frames does the same at
the end of a training run. The frames are made on the device (nerf/frames.py).
--video also writes results/ngp_rgb.avi and ngp_depth.avi, the reference's
ngp_rgb.mp4 / ngp_depth.mp4 (trainer.test(write_video=True)) as Motion-JPEG:
every frame is JPEG-encoded on the device (csrc/jpeg.hip, DESIGN.md section
19); --video_only leaves the PNGs out, --video_fps / --video_quality set the
rate (25) and the JPEG quality (90).
--bg_radius R > 0 adds the reference's background model (nerf/network.py
:107-129): what lies outside the box is learned as a colour per direction on
the sphere of radius R (a 2-D hash grid and a small MLP), trained against the
white-blended targets, and rendered in the evaluation and the frames.
--ema_decay D keeps the reference's exponential moving average of the
parameters (torch_ema, Trainer(ema_decay=0.95), main_nerf.py:219), updated at
the end of every epoch of len(train) steps (nerf/utils.py:1051-1052); the
evaluation, the frames and the best checkpoint then use the averaged weights,
as the reference's do, and ngp.pth carries them as `ema`. --eval_interval E
validates on the device every E epochs (nerf.eval.Validator over the val
split) and keeps the best model in <workspace>/checkpoints/ngp_best.pth
(--test --ckpt best renders it). --resume continues from
<workspace>/checkpoints/ngp.pth (or --ckpt PATH) to --iters. DESIGN.md
section 16. --ssim reports SSIM beside every PSNR (the periodic validation,
the final evaluation, and under --test the test split's own views), computed
on the device beside the squared error.

Not here: patch sampling, --color_space linear, more than one
image per batch, video files."""
import argparse
import math
import os
import sys
import time


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("path", type=str)
    p.add_argument("-O", action="store_true", help="fp16 + cuda_ray + preload: what this engine always runs")
    p.add_argument("--workspace", type=str, default="workspace")
    p.add_argument("--seed", type=int, default=0)
    # training options
    p.add_argument("--iters", type=int, default=30000, help="training iters")
    p.add_argument("--lr", type=float, default=1e-2, help="initial learning rate")
    p.add_argument("--num_rays", type=int, default=4096, help="num rays sampled per image for each training step")
    p.add_argument("--max_steps", type=int, default=1024, help="max num steps sampled per ray")
    p.add_argument("--update_extra_interval", type=int, default=16, help="iter interval to update the density grid")
    p.add_argument("--sample_budget", type=int, default=2 ** 20,
                   help="rows of the per-step sample buffers (the fixed M): rows past a step's sample count cost "
                        "nothing, rays past the budget are dropped for that step")
    # loss weights (the reference's opt.color_loss_weight / opt.depth_loss_weight)
    p.add_argument("--depth_loss_weight", type=float, default=0.0,
                   help="weight of the masked L1 depth loss (needs a dep_path per frame)")
    p.add_argument("--color_loss_weight", type=float, default=1.0, help="weight of the colour MSE")
    p.add_argument("--dist_loss_weight", type=float, default=0.0,
                   help="weight of the distortion regulariser on each ray's composite weights (the reference's "
                        "loss.py EffDistLoss; 0: off)")
    p.add_argument("--error_map", action="store_true", help="use error map to sample rays")
    p.add_argument("--error_map_res", type=int, default=128,
                   help="cells a side of each view's error map (1..128; needs num_rays <= its square)")
    # dataset options
    p.add_argument("--downscale", type=int, default=1)
    p.add_argument("--bound", type=float, default=2,
                   help="assume the scene is bounded in box[-bound, bound]^3, if > 1, will invoke adaptive ray marching.")
    p.add_argument("--scale", type=float, default=0.33, help="scale camera location into box[-bound, bound]^3")
    p.add_argument("--offset", type=float, nargs="*", default=[0, 0, 0], help="offset of camera location")
    p.add_argument("--depth_scale", type=float, default=None,
                   help="depth-map units to scene units, gt = depth * depth_scale (default: --scale)")
    p.add_argument("--dt_gamma", type=float, default=1 / 128,
                   help="dt_gamma (>=0) for adaptive ray marching. set to 0 to disable")
    p.add_argument("--min_near", type=float, default=0.2, help="minimum near distance for camera")
    p.add_argument("--density_thresh", type=float, default=10, help="threshold for density grid to be occupied")
    p.add_argument("--bg_radius", type=float, default=-1,
                   help="if positive, use a background model at sphere(bg_radius)")
    # mesh export (the reference's trainer.save_mesh(resolution=256, threshold=10), main_nerf.py:190 / :241)
    p.add_argument("--save_mesh", action="store_true", help="write <workspace>/meshes/ngp.ply after the evaluation")
    p.add_argument("--mesh_resolution", type=int, default=256, help="lattice points per axis of the mesh's volume")
    p.add_argument("--mesh_threshold", type=float, default=10, help="density at which the surface is drawn")
    p.add_argument("--mesh_color", action="store_true",
                   help="colour the mesh's vertices with the model's colour seen along the normal (red green blue)")
    p.add_argument("--mesh_min_faces", type=int, default=0,
                   help="drop connected components of the mesh with fewer triangles than this (0: off)")
    p.add_argument("--mesh_keep_largest", action="store_true",
                   help="keep only the connected component of the mesh with the most triangles")
    # EMA, validation while training, resuming (the reference's Trainer(ema_decay=0.95, eval_interval=...),
    # main_nerf.py:219, and its load_checkpoint on start, nerf/utils.py:410-432)
    p.add_argument("--ema_decay", type=float, default=None,
                   help="keep an exponential moving average of the parameters with this decay, updated every epoch, "
                        "and evaluate / save the best model with it (the reference trains with 0.95); default: off")
    p.add_argument("--eval_interval", type=int, default=0,
                   help="validate every this many epochs (an epoch is one step per training view) and keep the best "
                        "model in <workspace>/checkpoints/ngp_best.pth; 0: evaluate only at the end")
    p.add_argument("--ssim", action="store_true",
                   help="report SSIM (11 x 11 Gaussian window, sigma 1.5, valid region) beside PSNR, computed on the "
                        "device; the best checkpoint stays chosen by PSNR")
    p.add_argument("--resume", action="store_true",
                   help="continue training from <workspace>/checkpoints/ngp.pth (or --ckpt PATH) up to --iters")
    # test mode (the reference's --test / --ckpt and its trainer.test, main_nerf.py:188 / :239)
    p.add_argument("--test", action="store_true", help="test mode: load a checkpoint and write the test frames")
    p.add_argument("--ckpt", type=str, default="latest",
                   help="checkpoint --test (or --resume) loads; latest: <workspace>/checkpoints/ngp.pth, "
                        "best: <workspace>/checkpoints/ngp_best.pth")
    p.add_argument("--test_frames", type=int, default=10,
                   help="steps of the interpolated camera path when the scene has no transforms_test.json")
    p.add_argument("--write_frames", action="store_true",
                   help="after training and evaluation, write the test frames to <workspace>/results")
    # the test frames as video (the reference's trainer.test(write_video=True): ngp_rgb.mp4 / ngp_depth.mp4)
    p.add_argument("--video", action="store_true",
                   help="with --test or --write_frames: also write results/ngp_rgb.avi and ngp_depth.avi, "
                        "Motion-JPEG encoded on the device")
    p.add_argument("--video_fps", type=int, default=25, help="frames per second of the videos")
    p.add_argument("--video_quality", type=int, default=90, help="JPEG quality of the videos' frames, 1..100")
    p.add_argument("--video_only", action="store_true", help="the videos without the PNG files (implies --video)")
    return p


def _eval_split(path):
    for sp in ("val", "test"):
        if os.path.exists(os.path.join(path, f"transforms_{sp}.json")):
            return sp
    return "train"  # one transforms.json: the training views themselves


def _test_path(opt, train, dev, data_args):
    """The cameras of the test frames -> (poses [n, 4, 4], H, W, intrinsics,
    what they are, the test split's dataset or None): the test split's, or the
    reference's interpolation (provider.py:208-222) between two training poses
    drawn with --seed."""
    import numpy as np

    from nerf.provider import NeRFDataset, interpolate_poses
    # (NeRFDataset reads the splits only where there is no transforms.json)
    if not os.path.exists(os.path.join(opt.path, "transforms.json")) and \
            os.path.exists(os.path.join(opt.path, "transforms_test.json")):
        test = NeRFDataset(opt.path, dev, type="test", num_rays=opt.num_rays, **data_args)
        return test.poses, test.H, test.W, test.intrinsics, "test poses", test
    if train is None:  # --test: only the interpolated path needs the training views
        train = NeRFDataset(opt.path, dev, type="train", num_rays=opt.num_rays, **data_args)
    n = int(train.poses.shape[0])
    if n < 2 or opt.test_frames < 1:
        sys.exit(f"[main_nerf] no transforms_test.json under {opt.path}: a camera path needs two training poses "
                 f"(the scene has {n}) and --test_frames >= 1 (got {opt.test_frames})")
    a, b = np.random.default_rng(opt.seed).choice(n, 2, replace=False)
    poses = interpolate_poses(train.poses[a].cpu().numpy(), train.poses[b].cpu().numpy(), opt.test_frames)
    return poses, train.H, train.W, train.intrinsics, f"poses between training views {a} and {b}", None


def _ckpt_path(opt):
    name = {"latest": "ngp.pth", "best": "ngp_best.pth"}.get(opt.ckpt)
    return os.path.join(opt.workspace, "checkpoints", name) if name else opt.ckpt


def _ssim_validator(opt, model, data):
    """Validator(ssim=True) over `data`; a frame smaller than the window ends the run."""
    from nerf.eval import Validator
    try:
        return Validator(model, data, max_steps=opt.max_steps, dt_gamma=opt.dt_gamma, ssim=True)
    except ValueError as e:
        sys.exit(f"[main_nerf] --ssim: {e}")


def _write_test_frames(opt, model, train, dev, data_args, source=None, evaluate=False):
    """trainer.test (nerf/utils.py:743-796): every test pose rendered in eval
    mode on a white background, written under <workspace>/results. source: the
    weights to render instead of the model's own (the EMA's). evaluate (--test
    --ssim): the reference's trainer.evaluate(test_loader) where the frames are
    a split with images: its PSNR and SSIM, printed and added to the result."""
    import torch

    from nerf.frames import FrameRenderer, write_frames, write_video
    video = opt.video or opt.video_only
    if video and not 1 <= opt.video_quality <= 100:
        sys.exit(f"[main_nerf] --video_quality must be in 1..100, got {opt.video_quality}")
    if video and opt.video_fps < 1:
        sys.exit(f"[main_nerf] --video_fps must be at least 1, got {opt.video_fps}")
    poses, H, W, intrinsics, what, test = _test_path(opt, train, dev, data_args)
    was_training = model.training
    model.eval()
    fr = FrameRenderer(model, H, W, intrinsics, max_steps=opt.max_steps, dt_gamma=opt.dt_gamma, bg_color=1.0)
    fr.load_weights(source)
    fr.capture()
    fr.set_poses(poses)
    out_dir = os.path.join(opt.workspace, "results")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if video:
        videos, paths = write_video(fr, out_dir, "ngp", fps=opt.video_fps, quality=opt.video_quality,
                                    png=not opt.video_only)
    else:
        paths = write_frames(fr, out_dir, "ngp")
    secs = time.perf_counter() - t0
    model.train(was_training)
    print(f"[main_nerf] {len(fr)} frames {H}x{W} ({what}) in {secs:.2f} s, {len(fr) / secs:.1f} frames/s, "
          f"written to {out_dir}")
    result = {"frames": len(fr), "frames_per_second": len(fr) / secs, "results": out_dir, "frame_paths": paths}
    if video:
        print(f"[main_nerf] videos {videos[0]} and {videos[1]} ({opt.video_fps} frames/s, quality "
              f"{opt.video_quality})")
        result["video_paths"] = videos
    if evaluate and (test is None or getattr(test, "images", None) is None):
        print("[main_nerf] --ssim: the test frames have no images to compare with (an interpolated camera path)")
    elif evaluate:
        res = _ssim_validator(opt, model, test).run(source=source)
        print(f"[main_nerf] PSNR {res['mean_psnr']:.4f} over {len(res['views'])} test images")
        print(f"[main_nerf] SSIM {res['mean_ssim']:.4f} over {len(res['views'])} test images")
        result.update(psnr=res["mean_psnr"], ssim=res["mean_ssim"])
    return result


def _mesh_options(opt):
    """--mesh_color / --mesh_min_faces / --mesh_keep_largest as save_mesh keywords (none set: none passed) and
    the dict the cleaning fills."""
    info = {}
    if not (opt.mesh_color or opt.mesh_min_faces > 0 or opt.mesh_keep_largest):
        return {}, info
    return dict(colors=opt.mesh_color, min_faces=opt.mesh_min_faces, keep_largest=opt.mesh_keep_largest,
                info=info), info


def _mesh_report(opt, path, nv, nt, info, result):
    text = (f"[main_nerf] mesh {path}: {nv} vertices, {nt} triangles "
            f"(resolution {opt.mesh_resolution}, threshold {opt.mesh_threshold:g})")
    result.update(mesh=path, mesh_vertices=nv, mesh_triangles=nt)
    if info:
        text += (f", {info['components_kept']} of {info['components']} components kept "
                 f"({info['vertices_dropped']} vertices, {info['faces_dropped']} triangles dropped)")
        result.update(mesh_components=info["components"], mesh_components_kept=info["components_kept"])
    if opt.mesh_color:
        text += ", vertex colours"
    print(text)


def _test(opt, dev, bound, data_args):
    """--test: the model of a checkpoint, its frames and (--save_mesh) its mesh; nothing is trained."""
    import torch

    from nerf import mesh
    from nerf.network_ff import NeRFNetwork
    ckpt = _ckpt_path(opt)
    if not os.path.exists(ckpt):
        sys.exit(f"[main_nerf] --test: no checkpoint at {ckpt} (train first, or name one with --ckpt)")
    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    model = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, density_scale=1, min_near=opt.min_near,
                        density_thresh=opt.density_thresh, bg_radius=opt.bg_radius).to(dev)
    # the model part of FusedTrainer.load_checkpoint; the renderer marches density_bitfield itself
    model.load_state_dict(state.get("model", state), strict=False)
    model.mean_count = state.get("mean_count", model.mean_count)
    model.mean_density = state.get("mean_density", model.mean_density)
    # a full checkpoint of an EMA run: the averaged weights are what is rendered, as the reference's
    # trainer does after load_checkpoint (nerf/utils.py:1261-1262, 881-883); the mesh is the model's own
    source = None
    if isinstance(state.get("ema"), dict):
        source = [t.to(dev, torch.float32).contiguous() for t in state["ema"]["shadow_params"]]
    print(f"[main_nerf] checkpoint {ckpt} (step {state.get('global_step', '?')}"
          + (", EMA weights" if source is not None else "") + ")")
    result = {"checkpoint": ckpt}
    result.update(_write_test_frames(opt, model, None, dev, data_args, source, evaluate=opt.ssim))
    if opt.save_mesh:
        path = os.path.join(opt.workspace, "meshes", "ngp.ply")
        extra, info = _mesh_options(opt)
        nv, nt = mesh.save_mesh(model, path, resolution=opt.mesh_resolution, threshold=opt.mesh_threshold, **extra)
        _mesh_report(opt, path, nv, nt, info, result)
    return result


def main(argv=None):
    opt = get_parser().parse_args(argv)

    import torch

    from nerf.eval import Validator, depth_error, psnr, ray_distortion
    from nerf.fused import FusedTrainer
    from nerf.fused_render import FusedRenderer
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import NeRFDataset

    dev = torch.device("cuda:0")
    torch.manual_seed(opt.seed)
    bound = int(opt.bound) if float(opt.bound).is_integer() else opt.bound
    data_args = dict(downscale=opt.downscale, scale=opt.scale, offset=opt.offset, store="uint8",
                     depth_scale=opt.depth_scale)
    if opt.test:
        return _test(opt, dev, bound, data_args)
    state = None
    if opt.resume:
        ckpt = _ckpt_path(opt)
        if not os.path.exists(ckpt):
            sys.exit(f"[main_nerf] --resume: no checkpoint at {ckpt} (train first, or name one with --ckpt)")
        state = torch.load(ckpt, map_location="cpu", weights_only=False)
        if "optimizer" not in state:
            sys.exit(f"[main_nerf] --resume: {ckpt} holds no optimizer state (a best checkpoint): it can be "
                     "rendered with --test, not trained on")
    try:
        train = NeRFDataset(opt.path, dev, type="train", num_rays=opt.num_rays, error_map=opt.error_map,
                            error_map_res=opt.error_map_res, **data_args)
    except ValueError as e:  # e.g. an error map resolution out of range
        sys.exit(f"[main_nerf] {e}")
    model = NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, density_scale=1, min_near=opt.min_near,
                        density_thresh=opt.density_thresh, bg_radius=opt.bg_radius).to(dev)
    model.train()
    model.mark_untrained_grid(train.poses, train.intrinsics)
    M = (int(opt.sample_budget) + 127) // 128 * 128
    try:
        ft = FusedTrainer(model, train, M=M, lr=opt.lr, iters=opt.iters, max_steps=opt.max_steps,
                          dt_gamma=opt.dt_gamma, seed=opt.seed, depth_loss_weight=opt.depth_loss_weight,
                          color_loss_weight=opt.color_loss_weight, ema_decay=opt.ema_decay,
                          dist_loss_weight=opt.dist_loss_weight)
    except ValueError as e:  # e.g. a depth weight on a scene without depth maps
        sys.exit(f"[main_nerf] {e}")
    ema = opt.ema_decay is not None
    # an epoch is one step per training view (the reference's len(train_loader), batch size 1); the position
    # in it follows from the step count alone, so a checkpoint of a run that counted no epochs resumes right
    epoch_len = int(train.poses.shape[0])
    stats, done = None, 0
    if state is not None:
        ft.load_checkpoint(state)
        stats, done = state["stats"], int(state["global_step"])
        print(f"[main_nerf] resumed {ckpt} at step {done} (epoch {done // epoch_len}"
              + (f", {ft.num_updates} EMA updates" if ema else "") + ")")
        if ema and not isinstance(state.get("ema"), dict):
            # the shadow built with the trainer averages the initial weights: start it at the loaded ones
            ft.ema_reset()
            print(f"[main_nerf] {ckpt} carries no EMA: the average starts from its weights")
    start = done
    epoch, in_epoch = divmod(done, epoch_len)
    print(f"[main_nerf] {train.images.shape[0]} images {train.H}x{train.W}x{train.images.shape[3]} "
          f"({train.images.numel() / 2 ** 20:.0f} MiB uint8), {opt.num_rays} rays/step, sample budget {M}"
          + (f", error map {opt.error_map_res}x{opt.error_map_res}" if opt.error_map else "")
          + (f", background model at radius {opt.bg_radius:g} "
             f"({model.encoder_bg.embeddings.numel() + model.bg_net.weights.numel()} parameters)"
             if opt.bg_radius > 0 else ""))

    every = max(1, int(opt.update_extra_interval))
    log_every = max(every, opt.iters // 20 // every * every)
    over = torch.zeros((), dtype=torch.int64, device=dev)  # recorded steps whose samples passed the budget
    checked, captured = 0, False
    # epochs matter only to the EMA and the periodic validation: without both the loop below issues
    # today's calls
    use_epochs = ema or opt.eval_interval > 0
    split = _eval_split(opt.path)
    val, validator, ckpt_dir = None, None, os.path.join(opt.workspace, "checkpoints")
    if stats is None:
        stats = {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
    valid_psnr, valid_ssim, best_ckpt = [], [], None
    if opt.eval_interval > 0:
        val = train if split == "train" else NeRFDataset(opt.path, dev, type=split, num_rays=opt.num_rays,
                                                         **data_args)
        validator = _ssim_validator(opt, model, val) if opt.ssim else \
            Validator(model, val, max_steps=opt.max_steps, dt_gamma=opt.dt_gamma)

    def advance(k):
        nonlocal captured
        if captured:
            ft.run(k)
        else:
            for _ in range(k):  # the first interval eagerly, then the graphs
                ft.step()

    def end_epoch():
        """The reference's end of train_one_epoch / evaluate_one_epoch / save_checkpoint(best=True)
        (nerf/utils.py:1051-1052, 731-733, 1213-1233)."""
        nonlocal best_ckpt
        if ema:
            ft.ema_update()
        if validator is None or epoch % opt.eval_interval:
            return
        ft.flush()
        torch.cuda.synchronize()
        tv = time.perf_counter()
        res = validator.run(source=ft.ema_params() if ema else None)
        tv = time.perf_counter() - tv
        print(f"[main_nerf] epoch {epoch} validation PSNR {res['mean_psnr']:.4f}"
              + (f" SSIM {res['mean_ssim']:.4f}" if opt.ssim else "") + f" over {len(res['views'])} {split} "
              f"images ({tv:.3f} s)")
        stats["valid_loss"].append(res["mean_mse"])
        valid_psnr.append(res["mean_psnr"])
        if opt.ssim:
            valid_ssim.append(res["mean_ssim"])
        if stats["best_result"] is None or res["mean_psnr"] > stats["best_result"]:
            stats["best_result"] = res["mean_psnr"]
            best = ft.checkpoint(full=False, epoch=epoch, stats=stats)
            best["model"] = dict(best["model"])
            if ema:  # the averaged weights under the parameters' names
                names = {id(p): n for n, p in model.named_parameters()}
                for p, shadow in zip(ft.params, ft.ema_params()):
                    best["model"][names[id(p)]] = shadow.detach().cpu()  # (loads without a GPU)
            best["model"].pop("density_grid", None)  # (not trained on again, as the reference's)
            os.makedirs(ckpt_dir, exist_ok=True)
            best_ckpt = os.path.join(ckpt_dir, "ngp_best.pth")
            torch.save(best, best_ckpt)

    t0 = time.perf_counter()
    while done < opt.iters:
        # the reference's cadence (utils.py:580-582): an update at every interval's first step
        if done % every == 0:
            ft.update_density()
        k = min(every - done % every, opt.iters - done)
        if not use_epochs:
            advance(k)
        else:  # an interval that contains an epoch boundary runs in two parts
            left = k
            while left:
                part = min(left, epoch_len - in_epoch)
                advance(part)
                left, in_epoch = left - part, in_epoch + part
                if in_epoch == epoch_len:
                    epoch, in_epoch = epoch + 1, 0
                    end_epoch()
        if not captured and k == every and done + k < opt.iters:
            ft.capture(warmup=0, multi=max(every - 1, 1))
            captured = True
        done += k
        n = min(k, 16)
        over += ft.over_budget(n)
        checked += n
        if done % log_every == 0 or done == opt.iters:
            dep, dst = ft.last_depth_loss, ft.last_dist_loss  # None: the term is off
            terms = ""
            if dep is not None or dst is not None:
                terms = (f" (rgb {ft.last_color_loss:.6f}" + ("" if dep is None else f", dep {dep:.6f}")
                         + ("" if dst is None else f", dist {dst:.6f}") + ")")
            print(f"[main_nerf] step {done}/{opt.iters} loss {ft.last_loss:.6f}{terms} "
                  f"({time.perf_counter() - t0:.1f} s)")
    ft.flush()
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    errors = ft.device_errors()
    print(f"[main_nerf] trained {opt.iters - start} steps in {secs:.1f} s; {int(over.item())} of {checked} recorded "
          f"steps passed the sample budget of {M} rows (their last rays were dropped); device errors {errors}")

    # evaluation: the reference's eval_step over the val (or test) split
    # (with --ema_decay from the averaged weights, as every PSNR the reference reports is)
    if val is None:
        val = train if split == "train" else NeRFDataset(opt.path, dev, type=split, num_rays=opt.num_rays,
                                                         **data_args)
    model.eval()
    source = ft.ema_params() if ema else None
    renderer = validator.frames.renderer if validator is not None else \
        FusedRenderer(model, val.H * val.W, max_steps=opt.max_steps, dt_gamma=opt.dt_gamma)
    renderer.load_weights(source)
    scores = [psnr(model, val, i, dt_gamma=opt.dt_gamma, renderer=renderer) for i in range(val.poses.shape[0])]
    finite = [s for s in scores if math.isfinite(s)]
    mean_psnr = sum(finite) / len(finite) if finite else float("inf")
    print(f"[main_nerf] PSNR {mean_psnr:.4f} over {len(scores)} {split} images")
    # ... and, with --ssim, a device pass over the same views with the same weights
    mean_ssim = None
    if opt.ssim:
        res = (validator if validator is not None else _ssim_validator(opt, model, val)).run(source=source)
        mean_ssim = res["mean_ssim"]
        print(f"[main_nerf] SSIM {mean_ssim:.4f} over {len(res['views'])} {split} images")
    # ... and the supervised depth term over the same views, when the split has depth maps
    mean_depth = None
    if val.depths is not None:
        errs = [depth_error(model, val, i, dt_gamma=opt.dt_gamma, max_steps=opt.max_steps)
                for i in range(val.poses.shape[0])]
        errs = [e for e in errs if math.isfinite(e)]
        mean_depth = sum(errs) / len(errs) if errs else float("nan")
        print(f"[main_nerf] depth error {mean_depth:.6f} over {val.poses.shape[0]} {split} images")
    # ... and, with the distortion regulariser, what it regularises: the views' mean ray distortion
    mean_dist = None
    if opt.dist_loss_weight > 0:
        dists = [ray_distortion(model, val, i, dt_gamma=opt.dt_gamma, max_steps=opt.max_steps)
                 for i in range(val.poses.shape[0])]
        mean_dist = sum(dists) / len(dists)
        print(f"[main_nerf] ray distortion {mean_dist:.6f} over {val.poses.shape[0]} {split} images")
    model.train()

    os.makedirs(ckpt_dir, exist_ok=True)
    ckpt = os.path.join(ckpt_dir, "ngp.pth")
    state = ft.checkpoint(epoch=epoch if use_epochs else 0, stats=stats)
    state["stats"]["results"].append(mean_psnr)
    torch.save(state, ckpt)
    print(f"[main_nerf] checkpoint {ckpt}")
    result = {"psnr": mean_psnr, "loss": ft.last_loss, "over_budget": int(over.item()), "checkpoint": ckpt,
              "seconds": secs, "depth_error": mean_depth, "start_step": start, "epoch": epoch,
              "valid_psnr": valid_psnr, "best_checkpoint": best_ckpt, "dist_loss": ft.last_dist_loss,
              "ray_distortion": mean_dist}
    if opt.ssim:
        result.update(ssim=mean_ssim, valid_ssim=valid_ssim)
    if opt.save_mesh:
        ft.workspace = opt.workspace
        extra, info = _mesh_options(opt)
        path, nv, nt = ft.save_mesh(resolution=opt.mesh_resolution, threshold=opt.mesh_threshold, **extra)
        _mesh_report(opt, path, nv, nt, info, result)
    if opt.write_frames:
        result.update(_write_test_frames(opt, model, train, dev, data_args, source))
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
