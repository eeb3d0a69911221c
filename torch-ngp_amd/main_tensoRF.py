"""Train a TensoRF field on a scene (the reference's main_tensoRF.py).

    python main_tensoRF.py data/lego -O --workspace trial_tensorf --bound 1 --scale 0.8 --dt_gamma 0
    python main_tensoRF.py data/lego -O --workspace trial_tensorf --bound 1 --scale 0.8 --dt_gamma 0 --test

The field is the vector-matrix decomposition (tensoRF/network.py): three
planes and three lines for the density, three more of each for the colour
features, sampled and differentiated by csrc/tensorf.hip; the rays are marched
through the density grid and composited by the NeRFRenderer (-O is what runs:
fp16 autocast, the density grid, the images on the device). Training starts at
--resolution0 texels per axis and, at each step of --upsample_model_steps,
crops the box to the occupied cells and resamples every plane and line towards
--resolution1. It ends with the PSNR on the val (or test) split through
model.render and <workspace>/checkpoints/ngp.pth; --test loads that checkpoint
and evaluates. DESIGN.md §22.

Not included: --cp (network_cp) and CCNeRF; the background model (--bg_radius
> 0 exits); --patch_size / LPIPS and CLIP; the GUI; hipGraph capture;
data-parallel training; device-written test frames and video (the frame
renderer is bound to the fused network)."""
import argparse
import os
import sys
import time


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("path", type=str)
    p.add_argument("-O", action="store_true", help="fp16 + cuda_ray + preload: what always runs here")
    p.add_argument("--test", action="store_true", help="test mode: load the checkpoint and evaluate")
    p.add_argument("--workspace", type=str, default="workspace")
    p.add_argument("--seed", type=int, default=0)
    # training options
    p.add_argument("--iters", type=int, default=30000, help="training iters")
    p.add_argument("--lr0", type=float, default=2e-2, help="initial learning rate for embeddings")
    p.add_argument("--lr1", type=float, default=1e-3, help="initial learning rate for networks")
    p.add_argument("--num_rays", type=int, default=4096, help="num rays sampled per image for each training step")
    p.add_argument("--max_steps", type=int, default=1024, help="max num steps sampled per ray")
    p.add_argument("--update_extra_interval", type=int, default=16, help="iter interval to update the density grid")
    p.add_argument("--l1_reg_weight", type=float, default=1e-4, help="weight of the L1 penalty on the density set")
    # network options
    p.add_argument("--resolution0", type=int, default=128)
    p.add_argument("--resolution1", type=int, default=300)
    p.add_argument("--upsample_model_steps", type=int, nargs="*", default=[2000, 3000, 4000, 5500, 7000])
    # dataset options
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
    return p


def _eval_split(path):
    for sp in ("val", "test"):
        if os.path.exists(os.path.join(path, f"transforms_{sp}.json")):
            return sp
    return "train"  # one transforms.json: the training views themselves


def main(argv=None):
    opt = get_parser().parse_args(argv)
    if opt.bg_radius > 0:
        sys.exit("[main_tensoRF] --bg_radius: the background model is not included")
    print(opt)

    import torch

    from nerf.provider import NeRFDataset
    from tensoRF import NeRFNetwork, TensoRFTrainer, seed_everything

    seed_everything(opt.seed)
    dev = torch.device("cuda:0")
    bound = int(opt.bound) if float(opt.bound).is_integer() else opt.bound
    data_args = dict(downscale=opt.downscale, scale=opt.scale, offset=opt.offset, store="uint8",
                     num_rays=opt.num_rays)
    model = NeRFNetwork(resolution=[opt.resolution0] * 3, bound=bound, cuda_ray=True, density_scale=1,
                        min_near=opt.min_near, density_thresh=opt.density_thresh, bg_radius=opt.bg_radius).to(dev)
    print(model)
    split = _eval_split(opt.path)
    common = dict(workspace=opt.workspace, lr0=opt.lr0, lr1=opt.lr1, iters=opt.iters, dt_gamma=opt.dt_gamma,
                  max_steps=opt.max_steps, update_extra_interval=opt.update_extra_interval,
                  l1_reg_weight=opt.l1_reg_weight, upsample_model_steps=opt.upsample_model_steps,
                  resolution1=opt.resolution1)

    if opt.test:
        trainer = TensoRFTrainer(model, None, **common)
        if not os.path.exists(trainer.checkpoint_path()):
            sys.exit(f"[main_tensoRF] --test: no checkpoint at {trainer.checkpoint_path()} (train first)")
        state = trainer.load_checkpoint(model_only=True)
        print(f"[main_tensoRF] checkpoint {trainer.checkpoint_path()} (step {state['global_step']}, resolution "
              f"{model.resolution})")
        val = NeRFDataset(opt.path, dev, type=split, **data_args)
        mean_psnr, _ = trainer.evaluate(val)
        print(f"[main_tensoRF] PSNR {mean_psnr:.4f} over {val.poses.shape[0]} {split} images")
        return {"psnr": mean_psnr, "checkpoint": trainer.checkpoint_path(), "resolution": list(model.resolution)}

    train = NeRFDataset(opt.path, dev, type="train", **data_args)
    model.train()
    model.mark_untrained_grid(train.poses, train.intrinsics)
    trainer = TensoRFTrainer(model, train, **common)
    print(f"[main_tensoRF] upsample to {trainer.upsample_resolutions} at steps {trainer.upsample_model_steps}")
    t0 = time.perf_counter()
    trainer.train()
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print(f"[main_tensoRF] trained {trainer.global_step} steps in {secs:.1f} s, resolution {model.resolution}")
    val = train if split == "train" else NeRFDataset(opt.path, dev, type=split, **data_args)
    mean_psnr, _ = trainer.evaluate(val)
    print(f"[main_tensoRF] PSNR {mean_psnr:.4f} over {val.poses.shape[0]} {split} images")
    ckpt = trainer.save_checkpoint()
    print(f"[main_tensoRF] checkpoint {ckpt}")
    return {"psnr": mean_psnr, "checkpoint": ckpt, "seconds": secs, "resolution": list(model.resolution)}


if __name__ == "__main__":
    main(sys.argv[1:])
