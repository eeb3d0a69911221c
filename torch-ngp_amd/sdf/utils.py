"""SDFTrainer: the reference's sdf/utils.py Trainer as main_sdf.py:51-60 sets
it up, in the pattern of nerf/train.py: fp16 autocast and GradScaler, torch's
fused Adam (lr 1e-4, betas (0.9, 0.99), eps 1e-15, weight decay 1e-6 on the
MLP only), StepLR(10 epochs, 0.1), 20 epochs of 100 steps. The batch, its
signed distances and the loss are device work (sdf/provider.py, sdf/loss.py);
a step reads nothing back. Not included: EMA, hipGraph capture, data-parallel
training."""
import os
import random

import numpy as np
import torch

from .loss import mape_loss


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


class SDFTrainer:
    def __init__(self, model, dataset=None, workspace="workspace", lr=1e-4, epochs=20, steps_per_epoch=100,
                 fp16=True, name="ngp"):
        self.model, self.dataset, self.workspace, self.name = model, dataset, workspace, name
        self.epochs, self.steps_per_epoch, self.fp16 = int(epochs), int(steps_per_epoch), bool(fp16)
        self.optimizer = torch.optim.Adam([
            {"name": "encoding", "params": list(model.encoder.parameters())},
            {"name": "net", "params": list(model.backbone.parameters()), "weight_decay": 1e-6},
        ], lr=lr, betas=(0.9, 0.99), eps=1e-15, fused=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=10, gamma=0.1)
        self.scaler = torch.amp.GradScaler("cuda", enabled=self.fp16)
        self.epoch = 0
        self.global_step = 0
        self.losses = []  # device scalars of the steps since the last epoch report

    # ------------------------------------------------------------------ training
    def train_step(self):
        """One step on a fresh batch; returns the (device) loss."""
        self.model.train()
        self.optimizer.zero_grad(set_to_none=True)
        data = self.dataset.sample()
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            pred = self.model(data["points"])
        loss = mape_loss(pred, data["sdfs"])
        self.scaler.scale(loss).backward()
        self.scaler.step(self.optimizer)
        self.scaler.update()
        self.global_step += 1
        return loss.detach()

    def train_one_epoch(self):
        losses = [self.train_step() for _ in range(self.steps_per_epoch)]
        self.scheduler.step()
        self.epoch += 1
        return float(torch.stack(losses).mean().item())  # the epoch's one host read

    def train(self, epochs=None, log=print):
        for _ in range(self.epoch, self.epochs if epochs is None else int(epochs)):
            mean = self.train_one_epoch()
            err = self.evaluate()
            if log:
                log(f"==> epoch {self.epoch}: loss {mean:.6f}, |pred - sdf| {err:.6f}, "
                    f"lr {self.optimizer.param_groups[0]['lr']:.2e}")
            self.save_checkpoint()

    @torch.no_grad()
    def predict(self, points):
        """The network's sdf at points f32 [n, 3] -> f32 [n] (inference kernels)."""
        self.model.eval()
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.fp16):
            return self.model(points).float().reshape(-1)

    @torch.no_grad()
    def evaluate(self):
        """mean |pred - sdf| on a freshly drawn batch."""
        data = self.dataset.sample()
        pred = self.predict(data["points"])
        return float((pred - data["sdfs"].reshape(-1)).abs().mean().item())

    # --------------------------------------------------------------- checkpoints
    def checkpoint_path(self):
        return os.path.join(self.workspace, "checkpoints", f"{self.name}.pth")

    def save_checkpoint(self):
        path = self.checkpoint_path()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"epoch": self.epoch, "global_step": self.global_step, "model": self.model.state_dict(),
                    "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                    "scaler": self.scaler.state_dict()}, path)
        return path

    def load_checkpoint(self, model_only=False):
        path = self.checkpoint_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"no checkpoint at {path}")
        ck = torch.load(path, map_location=next(self.model.parameters()).device)
        self.model.load_state_dict(ck["model"])
        self.epoch, self.global_step = int(ck["epoch"]), int(ck["global_step"])
        if not model_only:
            self.optimizer.load_state_dict(ck["optimizer"])
            self.scheduler.load_state_dict(ck["scheduler"])
            self.scaler.load_state_dict(ck["scaler"])

    # ----------------------------------------------------------------------- mesh
    @torch.no_grad()
    def sdf_volume(self, resolution, chunk=2 ** 20):
        """The network on the resolution^3 lattice of [-1, 1]^3 -> f32 [R, R, R], in chunks."""
        from nerf.mesh import lattice_points
        R = int(resolution)
        N, dev = R ** 3, next(self.model.parameters()).device
        chunk = max(1, min(int(chunk), N))
        xyzs = torch.empty(chunk, 3, device=dev)
        volume = torch.empty(N, device=dev)
        aabb = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
        for lo in range(0, N, chunk):
            hi = min(lo + chunk, N)
            volume[lo:hi] = self.predict(lattice_points((R, R, R), aabb, lo, hi, xyzs))
        return volume.view(R, R, R)

    @torch.no_grad()
    def save_mesh(self, path, resolution=512):
        """The zero level set as a binary PLY -> (vertices, triangles). The
        volume marched is -sdf at threshold 0: inside is above the threshold,
        as nerf.mesh.marching_cubes wants it, so the normals point outwards."""
        from nerf.mesh import marching_cubes, write_ply
        volume = self.sdf_volume(resolution).neg_()
        verts, faces = marching_cubes(volume, 0.0, aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        write_ply(path, verts.cpu().numpy(), faces.cpu().numpy())
        return int(verts.shape[0]), int(faces.shape[0])
