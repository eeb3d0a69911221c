"""Train a dynamic scene, D-NeRF style (the reference's main_dnerf.py).

    python main_dnerf.py data/dnerf/jumpingjacks -O --workspace trial_dnerf --bound 1 --scale 0.8 --dt_gamma 0
    python main_dnerf.py data/dnerf/jumpingjacks -O --workspace trial_dnerf --bound 1 --scale 0.8 --dt_gamma 0 --test

The field is the hash grid behind a deformation MLP of (position, time)
(dnerf/network.py); every frame has a time, and the rays of a frame are
marched through the occupancy grid of its time slice, one of 64, all updated on
the device by csrc/dnerf.hip (-O is what runs: fp16 autocast, the density
grids, the images on the device). Training ends with the PSNR on the val (or
test) split, <workspace>/checkpoints/ngp.pth and the test poses rendered at
their times to <workspace>/results/ngp_<i>_rgb.png and _depth.png; --test loads
the checkpoint and renders them again. DESIGN.md §23.

Not included, and rejected where an option names them: --basis and --hyper,
the GUI, the background model (--bg_radius > 0), --error_map, --patch_size > 1,
CLIP guidance and random poses, the non-cuda_ray path; nor EMA, the fused
engine and hipGraph capture, data-parallel training, device-written frames and
video, save_mesh."""
import argparse
import os
import sys
import time


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("path", type=str)
    p.add_argument("-O", action="store_true", help="fp16 + cuda_ray + preload: what always runs here")
    p.add_argument("--test", action="store_true", help="test mode: load the checkpoint and render the test poses")
    p.add_argument("--workspace", type=str, default="workspace")
    p.add_argument("--seed", type=int, default=0)
    # training options
    p.add_argument("--iters", type=int, default=30000, help="training iters")
    p.add_argument("--lr", type=float, default=1e-2, help="initial learning rate of the hash grid")
    p.add_argument("--lr_net", type=float, default=1e-3, help="initial learning rate of the networks")
    p.add_argument("--ckpt", type=str, default="latest", help="'latest' (resume from ngp.pth if present), 'scratch' or a file")
    p.add_argument("--num_rays", type=int, default=4096, help="num rays sampled per image for each training step")
    p.add_argument("--cuda_ray", action="store_true", help="accepted: the only path here")
    p.add_argument("--max_steps", type=int, default=1024, help="max num steps sampled per ray")
    p.add_argument("--update_extra_interval", type=int, default=100, help="iter interval to update the density grids")
    p.add_argument("--patch_size", type=int, default=1, help="rejected above 1: no patch sampling here")
    # network options
    p.add_argument("--fp16", action="store_true", help="accepted: fp16 autocast always runs")
    p.add_argument("--basis", action="store_true", help="rejected: the temporal-basis network is not included")
    p.add_argument("--hyper", action="store_true", help="rejected: the hyper-nerf network is not included")
    p.add_argument("--time_size", type=int, default=64, help="time slices of the density grid (the reference's fixed 64)")
    p.add_argument("--grid_size", type=int, default=128, help="cells per axis of a density grid (a power of two)")
    # dataset options
    p.add_argument("--preload", action="store_true", help="accepted: the images always live on the device")
    p.add_argument("--downscale", type=int, default=1)
    p.add_argument("--bound", type=float, default=2,
                   help="assume the scene is bounded in box[-bound, bound]^3, if > 1, will invoke adaptive ray marching.")
    p.add_argument("--scale", type=float, default=0.33, help="scale camera location into box[-bound, bound]^3")
    p.add_argument("--offset", type=float, nargs="*", default=[0, 0, 0], help="offset of camera location")
    p.add_argument("--dt_gamma", type=float, default=1 / 128,
                   help="dt_gamma (>=0) for adaptive ray marching. set to 0 to disable")
    p.add_argument("--min_near", type=float, default=0.2, help="minimum near distance for camera")
    p.add_argument("--density_thresh", type=float, default=10, help="threshold for density grid to be occupied")
    p.add_argument("--bg_radius", type=float, default=-1, help="rejected when positive: no background model here")
    # rejected options of the reference
    p.add_argument("--gui", action="store_true", help="rejected: no GUI here")
    p.add_argument("--error_map", action="store_true", help="rejected: no error-map sampling here")
    p.add_argument("--clip_text", type=str, default="", help="rejected: no CLIP guidance here")
    p.add_argument("--rand_pose", type=int, default=-1, help="rejected when >= 0: no random poses here")
    return p


def reject_unsupported(opt):
    for flag, on, what in (("--basis", opt.basis, "the temporal-basis network is not included"),
                           ("--hyper", opt.hyper, "the hyper-nerf network is not included"),
                           ("--gui", opt.gui, "the GUI is not included"),
                           ("--bg_radius", opt.bg_radius > 0, "the background model is not included"),
                           ("--error_map", opt.error_map, "error-map sampling is not included"),
                           ("--patch_size", opt.patch_size > 1, "patch sampling is not included"),
                           ("--clip_text", bool(opt.clip_text), "CLIP guidance is not included"),
                           ("--rand_pose", opt.rand_pose >= 0, "random poses are not included")):
        if on:
            sys.exit(f"[main_dnerf] {flag}: {what}")


def _split(path, names):
    for sp in names:
        if os.path.exists(os.path.join(path, f"transforms_{sp}.json")):
            return sp
    return "train"  # one transforms.json: the training views themselves


def main(argv=None):
    opt = get_parser().parse_args(argv)
    reject_unsupported(opt)
    print(opt)

    import torch

    from dnerf import DNeRFTrainer, NeRFDataset, NeRFNetwork, seed_everything

    seed_everything(opt.seed)
    dev = torch.device("cuda:0")
    bound = int(opt.bound) if float(opt.bound).is_integer() else opt.bound
    data_args = dict(downscale=opt.downscale, scale=opt.scale, offset=opt.offset, store="uint8",
                     num_rays=opt.num_rays)
    model = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=opt.min_near,
                        density_thresh=opt.density_thresh, bg_radius=opt.bg_radius, time_size=opt.time_size,
                        grid_size=opt.grid_size).to(dev)
    model.grid_seed = opt.seed
    print(model)
    common = dict(workspace=opt.workspace, lr=opt.lr, lr_net=opt.lr_net, iters=opt.iters, dt_gamma=opt.dt_gamma,
                  max_steps=opt.max_steps, update_extra_interval=opt.update_extra_interval)
    test_split = _split(opt.path, ("test", "val"))

    def resume(trainer, required):
        path = trainer.checkpoint_path() if opt.ckpt in ("latest", "scratch") else opt.ckpt
        if opt.ckpt == "scratch" and not required:
            return None
        if not os.path.exists(path):
            if required or opt.ckpt != "latest":
                sys.exit(f"[main_dnerf] no checkpoint at {path}" + (" (train first)" if required else ""))
            return None
        state = trainer.load_checkpoint(path, model_only=required)
        print(f"[main_dnerf] checkpoint {path} (step {state['global_step']})")
        return state

    if opt.test:
        trainer = DNeRFTrainer(model, None, **common)
        resume(trainer, required=True)
        test = NeRFDataset(opt.path, dev, type=test_split, **data_args)
        files = trainer.test(test)
        print(f"[main_dnerf] wrote {len(files)} files for {test.poses.shape[0]} {test_split} poses")
        return {"files": files, "checkpoint": trainer.checkpoint_path()}

    train = NeRFDataset(opt.path, dev, type="train", **data_args)
    model.train()
    trainer = DNeRFTrainer(model, train, **common)
    if resume(trainer, required=False) is None:
        model.mark_untrained_grid(train.poses, train.intrinsics)
    t0 = time.perf_counter()
    trainer.train()
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print(f"[main_dnerf] trained to step {trainer.global_step} in {secs:.1f} s")
    val_split = _split(opt.path, ("val", "test"))
    val = train if val_split == "train" else NeRFDataset(opt.path, dev, type=val_split, **data_args)
    mean_psnr, _ = trainer.evaluate(val)
    print(f"[main_dnerf] PSNR {mean_psnr:.4f} over {val.poses.shape[0]} {val_split} images")
    ckpt = trainer.save_checkpoint()
    print(f"[main_dnerf] checkpoint {ckpt}")
    test = val if test_split == val_split else (train if test_split == "train" else
                                                NeRFDataset(opt.path, dev, type=test_split, **data_args))
    files = trainer.test(test)
    print(f"[main_dnerf] wrote {len(files)} files for {test.poses.shape[0]} {test_split} poses")
    return {"psnr": mean_psnr, "checkpoint": ckpt, "seconds": secs, "files": files}


if __name__ == "__main__":
    main(sys.argv[1:])
