"""TensoRFTrainer: the reference's tensoRF/utils.py Trainer as main_tensoRF.py
sets it up, in the pattern of nerf/train.py and sdf/utils.py: fp16 autocast
and GradScaler, torch's fused Adam (betas (0.9, 0.99), eps 1e-15) with lr0 on
the planes and lines and lr1 on basis_mat and the MLP, the 0.1 ** min(it /
iters, 1) schedule stepped every iteration, the colour MSE plus l1_reg_weight
* density_loss(), a density-grid update at every update_extra_interval-th
step's start, and at each step of upsample_model_steps: shrink_model, the new
resolution from the voxel budget, upsample_model, and a fresh optimizer and
scheduler (the parameters are new tensors). Not included: EMA, hipGraph
capture, data-parallel training, patch sampling, the background model
(DESIGN.md §22)."""
import math
import os
import random

import numpy as np
import torch

from .network import upsample_resolution, upsample_schedule


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


class TensoRFTrainer:
    def __init__(self, model, dataset=None, workspace="workspace", lr0=2e-2, lr1=1e-3, iters=30000, fp16=True,
                 dt_gamma=0.0, max_steps=1024, update_extra_interval=16, l1_reg_weight=1e-4,
                 upsample_model_steps=(), upsample_resolutions=None, resolution1=300, perturb=True, name="ngp",
                 log=print):
        """upsample_resolutions: the target of each step of upsample_model_steps
        (default: upsample_schedule from the model's first resolution to
        resolution1)."""
        self.model, self.dataset, self.workspace, self.name, self.log = model, dataset, workspace, name, log
        self.lr0, self.lr1, self.iters, self.fp16 = float(lr0), float(lr1), int(iters), bool(fp16)
        self.dt_gamma, self.max_steps, self.perturb = dt_gamma, int(max_steps), bool(perturb)
        self.update_extra_interval = int(update_extra_interval)
        self.l1_reg_weight = float(l1_reg_weight)
        self.upsample_model_steps = [int(s) for s in upsample_model_steps]
        if upsample_resolutions is None:
            upsample_resolutions = upsample_schedule(model.resolution[0], resolution1, len(self.upsample_model_steps))
        self.upsample_resolutions = [int(r) for r in upsample_resolutions]
        if len(self.upsample_resolutions) != len(self.upsample_model_steps):
            raise ValueError("TensoRFTrainer: one target resolution per upsample step")
        self.scaler = torch.amp.GradScaler("cuda", enabled=self.fp16)
        self.global_step = 0
        self.upsamples_done = 0
        self._reset_optimizer()

    def _reset_optimizer(self):
        """A new Adam and schedule over the model's current parameters (the schedule starts over, as the
        reference's lr_scheduler_fn(optimizer) does)."""
        self.optimizer = torch.optim.Adam(self.model.get_params(self.lr0, self.lr1), betas=(0.9, 0.99), eps=1e-15,
                                          fused=True)
        iters = self.iters
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lambda it: 0.1 ** min(it / iters, 1))

    # ------------------------------------------------------------------ training
    def _loss(self, data):
        images = data["images"]
        if images.shape[-1] == 4:  # a random background per pixel (the reference's bg_color for RGBA)
            bg_color = torch.rand_like(images[..., :3])
            gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
        else:
            bg_color, gt_rgb = 1, images
        outputs = self.model.render(data["rays_o"], data["rays_d"], staged=False, bg_color=bg_color,
                                    perturb=self.perturb, force_all_rays=False, dt_gamma=self.dt_gamma,
                                    max_steps=self.max_steps)
        loss = ((outputs["image"] - gt_rgb) ** 2).mean()
        if self.l1_reg_weight > 0:
            loss = loss + self.l1_reg_weight * self.model.density_loss()
        return loss

    def upsample(self):
        """One step of the schedule: shrink (density-grid models), the new
        resolution from the voxel budget inside aabb_train, upsample, and a
        fresh optimizer and scheduler."""
        if self.model.cuda_ray:
            self.model.shrink_model(log=self.log)
        n_vox = self.upsample_resolutions[self.upsamples_done] ** 3
        reso = upsample_resolution(self.model.aabb_train.cpu().numpy(), n_vox)
        if self.log:
            self.log(f"[INFO] upsample model at step {self.global_step} from {self.model.resolution} to {reso}")
        self.model.upsample_model(reso)
        self.upsamples_done += 1
        self._reset_optimizer()

    def train_step(self):
        """One step on a fresh batch; returns the (device) loss."""
        self.model.train()
        if self.model.cuda_ray and self.global_step % self.update_extra_interval == 0:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                self.model.update_extra_state()
        self.global_step += 1
        self.optimizer.zero_grad(set_to_none=True)
        data = self.dataset.sample()
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            loss = self._loss(data)
        self.scaler.scale(loss).backward()
        self.scaler.step(self.optimizer)
        self.scaler.update()
        self.scheduler.step()
        if self.global_step in self.upsample_model_steps:
            self.upsample()
        return loss.detach()

    def train(self, iters=None, log_every=None):
        iters = self.iters if iters is None else int(iters)
        log_every = log_every or max(1, iters // 20)
        losses = []
        while self.global_step < iters:
            losses.append(self.train_step())
            if self.log and (self.global_step % log_every == 0 or self.global_step == iters):
                mean = float(torch.stack(losses).mean().item())  # the report's one host read
                losses = []
                self.log(f"[tensoRF] step {self.global_step}/{iters} loss {mean:.6f} "
                         f"lr {self.optimizer.param_groups[0]['lr']:.2e}")

    # ---------------------------------------------------------------- evaluation
    @torch.no_grad()
    def render_view(self, dataset, index, chunk=4096):
        """All H * W rays of pose `index` through model.render in eval mode on white -> image [H * W, 3]."""
        from nerf.utils import get_rays
        H, W = int(dataset.H), int(dataset.W)
        rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
        was_training = self.model.training
        self.model.eval()
        out = []
        try:
            for a in range(0, H * W, chunk):
                with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                    r = self.model.render(rays["rays_o"][:, a:a + chunk], rays["rays_d"][:, a:a + chunk],
                                          staged=False, bg_color=1, perturb=False, dt_gamma=self.dt_gamma,
                                          max_steps=self.max_steps)
                out.append(r["image"].float().reshape(-1, 3))
        finally:
            self.model.train(was_training)
        return torch.cat(out)

    @torch.no_grad()
    def evaluate(self, dataset):
        """Mean PSNR over the dataset's views (nerf.eval.ground_truth: RGBA on white), the views with a
        finite PSNR as main_nerf takes it -> (mean, per view)."""
        from nerf.eval import ground_truth
        scores = []
        for i in range(int(dataset.poses.shape[0])):
            mse = float(((self.render_view(dataset, i) - ground_truth(dataset, i)) ** 2).mean().item())
            scores.append(-10.0 * math.log10(mse) if mse > 0 else float("inf"))
        finite = [s for s in scores if math.isfinite(s)]
        return (sum(finite) / len(finite) if finite else float("inf")), scores

    # --------------------------------------------------------------- checkpoints
    def checkpoint_path(self):
        return os.path.join(self.workspace, "checkpoints", f"{self.name}.pth")

    def save_checkpoint(self, path=None):
        """The model in the reference's layout with its resolution and
        aabb_train, the density-grid statistics, and the training state."""
        path = path or self.checkpoint_path()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        m = self.model
        state = {"global_step": self.global_step, "upsamples_done": self.upsamples_done, "model": m.state_dict(),
                 "resolution": list(m.resolution), "aabb_train": m.aabb_train.detach().cpu(),
                 "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                 "scaler": self.scaler.state_dict()}
        if m.cuda_ray:
            state["mean_count"], state["mean_density"] = m.mean_count, m.mean_density
        torch.save(state, path)
        return path

    def load_checkpoint(self, path=None, model_only=False):
        """Restores a model of any resolution (its planes and lines take the
        checkpoint's shapes); the optimizer is rebuilt over the new parameters
        before its state is loaded."""
        path = path or self.checkpoint_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"no checkpoint at {path}")
        m = self.model
        state = torch.load(path, map_location=next(m.parameters()).device, weights_only=False)
        m.load_state_dict(state["model"])
        if list(m.resolution) != [int(r) for r in state["resolution"]]:
            raise RuntimeError(f"checkpoint {path}: resolution {state['resolution']} but planes of {m.resolution}")
        if m.cuda_ray:
            m.mean_count = state.get("mean_count", m.mean_count)
            m.mean_density = state.get("mean_density", m.mean_density)
        self.global_step = int(state["global_step"])
        self.upsamples_done = int(state.get("upsamples_done", 0))
        self._reset_optimizer()
        if not model_only:
            self.optimizer.load_state_dict(state["optimizer"])
            self.scheduler.load_state_dict(state["scheduler"])
            self.scaler.load_state_dict(state["scaler"])
        return state
