"""Evaluation of a trained model against a dataset's images: the reference's
eval_step (nerf/utils.py:636-642) on the device-driven test render; and
against its depth maps: the supervised depth term over a whole view.
Validator is the same comparison kept on the device:
the frame renderer's rays and loop, then the squared error against the image
stack in one launch per view and one read-back per pass; with ssim=True a
second launch per view adds the view's SSIM, of which
ssim_reference is the definition."""
import ctypes
import math

import numpy as np
import torch

import _ngp_native as nat

from .frames import FrameRenderer
from .fused_render import FusedRenderer
from .utils import get_rays


def ground_truth(dataset, index):
    """Image `index` as the reference's eval_step compares it: RGB as stored,
    RGBA blended on white (bg_color = 1), float32 [H * W, 3]."""
    img = dataset.images[index]
    img = img.float() / torch.full((1,), 255.0, device=img.device) if img.dtype == torch.uint8 else img.float()
    img = img.reshape(-1, img.shape[-1])
    if img.shape[-1] == 4:
        return img[:, :3] * img[:, 3:] + (1 - img[:, 3:])
    return img


SSIM_WINDOW, SSIM_SIGMA = 11, 1.5
SSIM_C1, SSIM_C2 = 0.01 * 0.01, 0.03 * 0.03  # data range 1


def ssim_weights():
    """The window's 1-D weights: g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10,
    normalised to sum 1, float64."""
    k = np.arange(SSIM_WINDOW, dtype=np.float64) - (SSIM_WINDOW // 2)
    g = np.exp(-(k * k) / (2.0 * SSIM_SIGMA * SSIM_SIGMA))
    return g / g.sum()


def ssim_reference(x, y):
    """SSIM of two [H, W, 3] float32 images (x the render, y the ground truth)
    as ngp_frame_ssim defines it, in float64 numpy: Wang et al. 2004 with the
    11 x 11 Gaussian window (sigma 1.5) applied separably over the valid region
    (no padding), per channel; C1 = 0.01^2, C2 = 0.03^2, data range 1 (the form
    of mip-NeRF, pytorch_msssim, and skimage with gaussian_weights=True,
    use_sample_covariance=False and the borders cropped). -> (map float64
    [H - 10, W - 10, 3], its mean)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.ndim != 3 or x.shape[2] != 3 or x.dtype != np.float32 or y.dtype != np.float32:
        raise ValueError(f"ssim_reference: two float32 [H, W, 3] images, got {x.dtype} {list(x.shape)} and "
                         f"{y.dtype} {list(y.shape)}")
    H, W = x.shape[:2]
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f"ssim_reference: the 11 x 11 window needs H, W >= 11, got {H} x {W}")
    g = ssim_weights()
    x, y = x.astype(np.float64), y.astype(np.float64)

    def window(a):  # the windowed mean: along W, then along H
        h = sum(g[k] * a[:, k:k + W - SSIM_WINDOW + 1] for k in range(SSIM_WINDOW))
        return sum(g[k] * h[k:k + H - SSIM_WINDOW + 1] for k in range(SSIM_WINDOW))

    mux, muy = window(x), window(y)
    sx, sy, sxy = window(x * x) - mux * mux, window(y * y) - muy * muy, window(x * y) - mux * muy
    m = ((2.0 * mux * muy + SSIM_C1) * (2.0 * sxy + SSIM_C2)) / \
        ((mux * mux + muy * muy + SSIM_C1) * (sx + sy + SSIM_C2))
    return m, float(m.mean())


@torch.no_grad()
def psnr(model, dataset, index, dt_gamma=0.0, renderer=None):
    """PSNR (-10 log10 of the MSE over every pixel and channel) of the model's
    render of pose `index` against the dataset's image: all H * W rays of the
    pose (get_rays), rendered on a white background. renderer: a FusedRenderer
    of H * W rays with its weights loaded, to reuse one across calls."""
    H, W = int(dataset.H), int(dataset.W)
    if renderer is None:
        renderer = FusedRenderer(model, H * W, dt_gamma=dt_gamma)
        renderer.load_weights()
    rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
    out = renderer.render(rays["rays_o"], rays["rays_d"], bg_color=1)
    mse = float(((out["image"] - ground_truth(dataset, index)) ** 2).mean().item())
    return -10.0 * math.log10(mse) if mse > 0 else float("inf")


@torch.no_grad()
def depth_error(model, dataset, index, dt_gamma=0.0, max_steps=1024, chunk=4096):
    """Masked mean |gt - depth_bound_scale| over all H * W rays of pose `index`:
    the quantity depth supervision trains (nerf/utils.py:545-553), so it is
    computed with the training composite through the reference-API render
    (perturb=False, force_all_rays=True), the target dataset.depths[index] *
    depth_scale, the mask min_near <= gt <= bound. nan when no pixel of the
    view lies in the mask."""
    H, W = int(dataset.H), int(dataset.W)
    if getattr(dataset, "depths", None) is None:
        raise ValueError("depth_error: the dataset has no depth maps (dataset.depths)")
    rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
    was_training = model.training
    model.train()  # the training composite (march_rays_train + composite_rays_train)
    local_step, counts = model.local_step, model.step_counter.clone()
    pred = []
    try:
        # force_all_rays sizes the sample buffers for max_steps samples per ray: a few thousand rays at a time
        for a in range(0, H * W, chunk):
            with torch.autocast("cuda", dtype=torch.float16):
                out = model.render(rays["rays_o"][:, a:a + chunk], rays["rays_d"][:, a:a + chunk], staged=False,
                                   bg_color=1, perturb=False, force_all_rays=True, dt_gamma=dt_gamma,
                                   max_steps=max_steps)
            pred.append(out["depth_bound_scale"].float())
    finally:
        # (run_cuda counted training steps: the trainer's bookkeeping stays as it was)
        model.local_step = local_step
        model.step_counter.copy_(counts)
        model.train(was_training)
    gt = dataset.depths[index].reshape(1, -1) * dataset.depth_scale
    mask = (model.min_near <= gt) & (gt <= model.bound)
    err = torch.abs(gt - torch.cat(pred, 1))[mask]
    return float(err.mean().item()) if err.numel() else float("nan")


@torch.no_grad()
def ray_distortion(model, dataset, index, dt_gamma=0.0, max_steps=1024, chunk=4096):
    """Mean distortion term (the reference's loss.py EffDistLoss on the
    composite's weights, in ngp units; 0 for a ray without samples) over all
    H * W rays of pose `index`: the quantity dist_loss_weight regularises, so it
    is computed with the training composite through the reference-API render
    (perturb=False, force_all_rays=True, dist_loss=True), in the manner of
    depth_error."""
    H, W = int(dataset.H), int(dataset.W)
    rays = get_rays(dataset.poses[index:index + 1], dataset.intrinsics, H, W, -1)
    was_training = model.training
    model.train()  # the training composite (march_rays_train + distortion_rays_train)
    local_step, counts = model.local_step, model.step_counter.clone()
    total = torch.zeros((), dtype=torch.float64, device=rays["rays_o"].device)
    try:
        for a in range(0, H * W, chunk):
            with torch.autocast("cuda", dtype=torch.float16):
                out = model.render(rays["rays_o"][:, a:a + chunk], rays["rays_d"][:, a:a + chunk], staged=False,
                                   bg_color=1, perturb=False, force_all_rays=True, dt_gamma=dt_gamma,
                                   max_steps=max_steps, dist_loss=True)
            total += out["distortion"].double().sum()
    finally:
        # (run_cuda counted training steps: the trainer's bookkeeping stays as it was)
        model.local_step = local_step
        model.step_counter.copy_(counts)
        model.train(was_training)
    return float(total.item()) / (H * W)


class Validator:
    """The reference's evaluate_one_epoch (nerf/utils.py:1075-1173) over a
    dataset's views without leaving the device: a FrameRenderer over the
    dataset's poses and a [n_views] double buffer. Per view: ngp_frame_begin
    (the pose's rays), the render loop, ngp_frame_sse (the blend on white and
    the squared error against dataset.images[view], summed in double). The
    buffer is read back once per pass; the only other host synchronisation is
    the render loop's own 16-byte state read per graph replay. ssim=True: a
    second [n_views] double buffer and, after ngp_frame_sse on the same render,
    ngp_frame_ssim (the sum of the view's SSIM map),
    read back with the first."""

    def __init__(self, model, dataset, max_steps=1024, dt_gamma=0.0, ssim=False):
        images = getattr(dataset, "images", None)
        if images is None:
            raise ValueError("Validator: the dataset has no images (dataset.images)")
        self.model, self.data = model, dataset
        self.H, self.W = int(dataset.H), int(dataset.W)
        self.n = int(dataset.poses.shape[0])
        if ssim and (self.H < SSIM_WINDOW or self.W < SSIM_WINDOW):
            raise ValueError(f"Validator: SSIM's 11 x 11 window needs H, W >= 11, the dataset is {self.H} x {self.W}")
        self.frames = FrameRenderer(model, self.H, self.W, dataset.intrinsics, max_steps=max_steps,
                                    dt_gamma=dt_gamma, bg_color=1.0)
        dev = self.frames.dev
        if images.dim() != 4 or tuple(images.shape[:3]) != (self.n, self.H, self.W) or images.shape[3] not in (3, 4):
            raise ValueError(f"Validator: dataset.images must be [n_poses, H, W, 3 or 4] = "
                             f"[{self.n}, {self.H}, {self.W}, 3 | 4], got {list(images.shape)}")
        if images.dtype not in (torch.uint8, torch.float32) or not images.is_contiguous() or images.device != dev:
            raise ValueError(f"Validator: dataset.images must be contiguous uint8 or float32 on {dev}, got "
                             f"{images.dtype} on {images.device}")
        self._images = images  # (kept alive with its pointer)
        self._src = nat.ImageSource()
        self._src.pixels, self._src.channels = nat.ptr(images), int(images.shape[3])
        self._src.dtype = nat.DTYPE_U8 if images.dtype == torch.uint8 else nat.DTYPE_CODE[torch.float32]
        self.frames.set_poses(dataset.poses)
        self.sse = torch.zeros(self.n, dtype=torch.float64, device=dev)
        self.ssim = torch.zeros(self.n, dtype=torch.float64, device=dev) if ssim else None  # sums of the maps

    def sse_view(self, i):
        """View i rendered with the loaded weights, its squared error into
        self.sse[i] and, with ssim, the sum of its SSIM map into self.ssim[i]
        (no read-back)."""
        fr = self.frames
        r, P = fr.renderer, nat.ptr
        fr.begin(i)
        r.run_loop()
        bg_color = fr.bg_color
        if r._bg:  # as FrameRenderer.render: the model's background blended in place, then nothing to add
            r.background(blend=True)
            bg_color = 0.0
        nat.check(nat.lib().ngp_frame_sse(self.H, self.W, P(r.image), P(r.weights_sum), bg_color,
                                          ctypes.byref(self._src), i, P(self.sse), r._stream()), "frame_sse")
        if self.ssim is not None:
            nat.check(nat.lib().ngp_frame_ssim(self.H, self.W, P(r.image), P(r.weights_sum), bg_color,
                                               ctypes.byref(self._src), i, P(self.ssim), None, r._stream()),
                      "frame_ssim")

    @torch.no_grad()
    def run(self, source=None, views=None):
        """Every view (or `views`, a list of indices) of the dataset rendered
        in eval mode from `source` (FusedRenderer.load_weights: None, the
        model's own weights; FusedTrainer.ema_params(), the averaged ones) ->
        dict(views, mse, psnr: float64 arrays by position in views; mean_mse;
        mean_psnr, over the views with a finite PSNR as main_nerf's final
        evaluation takes it). mse = sse / (3 H W), psnr = -10 log10(mse). With
        ssim=True also ssim (float64 by position in views: the mean of each
        view's SSIM map) and mean_ssim (their plain mean)."""
        views = list(range(self.n)) if views is None else [int(v) for v in views]
        for v in views:
            if not 0 <= v < self.n:
                raise IndexError(f"Validator: view {v} of {self.n}")
        was_training = self.model.training
        self.model.eval()
        try:
            self.frames.load_weights(source)
            if self.frames.renderer.graph is None:
                self.frames.capture()
            for v in views:
                self.sse_view(v)
        finally:
            self.model.train(was_training)
        if self.ssim is None:
            sse = self.sse.cpu().numpy()[views]  # the pass's one read-back
        else:  # ... of both buffers in one copy
            both = torch.stack((self.sse, self.ssim)).cpu().numpy()
            halo = SSIM_WINDOW - 1  # the map has (H - 10) (W - 10) positions per channel
            sse, ssim_ = both[0][views], both[1][views] / float(3 * (self.H - halo) * (self.W - halo))
        mse = sse / float(3 * self.H * self.W)
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr_ = np.where(mse > 0, -10.0 * np.log10(mse), np.inf)
        psnr_ = np.where(np.isfinite(mse), psnr_, np.nan)
        finite = psnr_[np.isfinite(psnr_)]
        res = {"views": views, "mse": mse, "psnr": psnr_,
               "mean_mse": float(mse.mean()) if len(views) else float("nan"),
               "mean_psnr": float(finite.mean()) if finite.size else float("inf")}
        if self.ssim is not None:
            res.update(ssim=ssim_, mean_ssim=float(ssim_.mean()) if len(views) else float("nan"))
        return res
