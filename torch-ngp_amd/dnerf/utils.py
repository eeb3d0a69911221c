"""DNeRFTrainer: the reference's dnerf/utils.py Trainer as main_dnerf.py sets
it up, in the pattern of TensoRFTrainer: fp16 autocast and GradScaler, torch's
fused Adam (betas (0.9, 0.99), eps 1e-15) over get_params(lr, lr_net), the
0.1 ** min(it / iters, 1) schedule stepped every iteration, the colour MSE
plus 1e-3 * deform.abs().mean() (reference :48), and the time-sliced density
grid's update at every update_extra_interval-th step's start. Not included:
EMA, hipGraph capture, data-parallel training, patch sampling, the error map,
CLIP, the background model."""
import math
import os
import random

import numpy as np
import torch


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


class DNeRFTrainer:
    def __init__(self, model, dataset=None, workspace="workspace", lr=1e-2, lr_net=1e-3, iters=30000, fp16=True,
                 dt_gamma=0.0, max_steps=1024, update_extra_interval=100, deform_weight=1e-3, perturb=True,
                 name="ngp", log=print):
        self.model, self.dataset, self.workspace, self.name, self.log = model, dataset, workspace, name, log
        self.lr, self.lr_net, self.iters, self.fp16 = float(lr), float(lr_net), int(iters), bool(fp16)
        self.dt_gamma, self.max_steps, self.perturb = dt_gamma, int(max_steps), bool(perturb)
        self.update_extra_interval = int(update_extra_interval)
        self.deform_weight = float(deform_weight)
        self.scaler = torch.amp.GradScaler("cuda", enabled=self.fp16)
        self.global_step = 0
        self.optimizer = torch.optim.Adam(model.get_params(self.lr, self.lr_net), betas=(0.9, 0.99), eps=1e-15,
                                          fused=True)
        iters_ = self.iters
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lambda it: 0.1 ** min(it / iters_, 1))

    # ------------------------------------------------------------------ training
    def losses(self, data):
        """(colour MSE, deformation penalty) of a batch, both on the device."""
        images = data["images"]
        if images.shape[-1] == 4:  # a random background per pixel (the reference's bg_color for RGBA)
            bg_color = torch.rand_like(images[..., :3])
            gt_rgb = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])
        else:
            bg_color, gt_rgb = 1, images
        outputs = self.model.render(data["rays_o"], data["rays_d"], data["time"], staged=False, bg_color=bg_color,
                                    perturb=self.perturb, force_all_rays=False, dt_gamma=self.dt_gamma,
                                    max_steps=self.max_steps)
        mse = ((outputs["image"] - gt_rgb) ** 2).mean()
        deform = outputs["deform"]
        reg = deform.abs().mean() if deform.numel() else mse.new_zeros(())
        return mse, reg

    def train_step(self):
        """One step on a fresh batch; returns the (device) colour MSE."""
        self.model.train()
        if self.global_step % self.update_extra_interval == 0:
            with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                self.model.update_extra_state()
        self.global_step += 1
        self.optimizer.zero_grad(set_to_none=True)
        data = self.dataset.sample()
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            mse, reg = self.losses(data)
            loss = mse + self.deform_weight * reg
        self.scaler.scale(loss).backward()
        self.scaler.step(self.optimizer)
        self.scaler.update()
        self.scheduler.step()
        return mse.detach()

    def train(self, iters=None, log_every=None):
        iters = self.iters if iters is None else int(iters)
        log_every = log_every or max(1, iters // 20)
        losses = []
        while self.global_step < iters:
            losses.append(self.train_step())
            if self.log and (self.global_step % log_every == 0 or self.global_step == iters):
                mean = float(torch.stack(losses).mean().item())  # the report's one host read
                losses = []
                self.log(f"[dnerf] step {self.global_step}/{iters} mse {mean:.6f} "
                         f"lr {self.optimizer.param_groups[0]['lr']:.2e}")

    # ---------------------------------------------------------------- evaluation
    @torch.no_grad()
    def render_view(self, dataset, index, chunk=4096):
        """All H * W rays of pose `index` at its time, eval mode, on white -> image [H * W, 3], depth [H * W]."""
        from nerf.utils import get_rays
        H, W = int(dataset.H), int(dataset.W)
        rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
        time = dataset.times[index:index + 1]
        was_training = self.model.training
        self.model.eval()
        image, depth = [], []
        try:
            for a in range(0, H * W, chunk):
                with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
                    r = self.model.render(rays["rays_o"][:, a:a + chunk], rays["rays_d"][:, a:a + chunk], time,
                                          staged=False, bg_color=1, perturb=False, dt_gamma=self.dt_gamma,
                                          max_steps=self.max_steps)
                image.append(r["image"].float().reshape(-1, 3))
                depth.append(r["depth"].float().reshape(-1))
        finally:
            self.model.train(was_training)
        return torch.cat(image), torch.cat(depth)

    @torch.no_grad()
    def evaluate(self, dataset):
        """Mean PSNR over the dataset's views at their times (RGBA on white) -> (mean, per view)."""
        from nerf.eval import ground_truth
        scores = []
        for i in range(int(dataset.poses.shape[0])):
            mse = float(((self.render_view(dataset, i)[0] - ground_truth(dataset, i)) ** 2).mean().item())
            scores.append(-10.0 * math.log10(mse) if mse > 0 else float("inf"))
        finite = [s for s in scores if math.isfinite(s)]
        return (sum(finite) / len(finite) if finite else float("inf")), scores

    @torch.no_grad()
    def test(self, dataset, save_path=None):
        """results/<name>_<i>_rgb.png and _depth.png for the dataset's poses at their times -> the files."""
        from PIL import Image
        save_path = save_path or os.path.join(self.workspace, "results")
        os.makedirs(save_path, exist_ok=True)
        H, W = int(dataset.H), int(dataset.W)
        files = []
        for i in range(int(dataset.poses.shape[0])):
            image, depth = self.render_view(dataset, i)
            rgb = (image.clamp(0, 1) * 255).round().to(torch.uint8).view(H, W, 3).cpu().numpy()
            dep = (depth.clamp(0, 1) * 255).round().to(torch.uint8).view(H, W).cpu().numpy()
            for arr, kind in ((rgb, "rgb"), (dep, "depth")):
                files.append(os.path.join(save_path, f"{self.name}_{i:04d}_{kind}.png"))
                Image.fromarray(arr).save(files[-1])
        return files

    # --------------------------------------------------------------- checkpoints
    def checkpoint_path(self):
        return os.path.join(self.workspace, "checkpoints", f"{self.name}.pth")

    def save_checkpoint(self, path=None):
        path = path or self.checkpoint_path()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        m = self.model
        torch.save({"global_step": self.global_step, "model": m.state_dict(), "mean_count": m.mean_count,
                    "mean_density": m.mean_density, "iter_density": m.iter_density,
                    "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                    "scaler": self.scaler.state_dict()}, path)
        return path

    def load_checkpoint(self, path=None, model_only=False):
        path = path or self.checkpoint_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"no checkpoint at {path}")
        m = self.model
        state = torch.load(path, map_location=next(m.parameters()).device, weights_only=False)
        m.load_state_dict(state["model"])
        m.mean_count = state.get("mean_count", m.mean_count)
        m.mean_density = state.get("mean_density", m.mean_density)
        m.iter_density = state.get("iter_density", m.iter_density)
        self.global_step = int(state["global_step"])
        if not model_only:
            self.optimizer.load_state_dict(state["optimizer"])
            self.scheduler.load_state_dict(state["scheduler"])
            self.scaler.load_state_dict(state["scaler"])
        return state
