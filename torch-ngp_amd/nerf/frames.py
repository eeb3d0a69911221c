"""Finished frames from a trained model: the reference's test render
(Trainer.test / test_step, nerf/utils.py:656-685, 743-796), which renders
every ray of each test pose, quantises colour and depth with
(x * 255).astype(np.uint8) and writes <name>_<i>_rgb.png / _depth.png.

Around the device-driven loop (nerf/fused_render.py) a frame is two launches
(csrc/frame.hip): ngp_frame_begin makes all H * W rays of one pose of a device
pose stack, their near / far and the loop's initial state (get_rays +
near_far_from_aabb + render_init, with no host-to-device copy per frame), and
ngp_frame_finish blends the background, normalises the depth and quantises
both to uint8, so 4 bytes per pixel leave the device instead of 16.

q(x) = uint8(clamp(x, 0, 1) * 255), truncating, 0 for a non-finite x: the
reference's cast, made total (a ray that misses the box has depth 0 / 0).

The reference's imageio.mimwrite (<name>_rgb.mp4 / _depth.mp4) needs an
encoder this project does not depend on; write_video keeps the same frames as
Motion-JPEG instead, <name>_rgb.avi / _depth.avi, encoded on the device
(csrc/jpeg.hip, nerf/jpeg.py, nerf/video.py), beside the PNG sequence or in
its place. DESIGN.md §14, §19."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import _ngp_native as nat

from .fused_render import FusedRenderer


def quantise(x):
    """q(x) on a numpy array: what ngp_frame_finish writes for the float x."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        y = np.clip(np.where(np.isfinite(x), x, np.float32(0)), np.float32(0), np.float32(1)) * np.float32(255)
    return y.astype(np.uint8)


class FrameRenderer:
    def __init__(self, model, H, W, intrinsics, max_steps=1024, dt_gamma=0.0, bg_color=1.0, iters_per_graph=8):
        self.model, self.H, self.W = model, int(H), int(W)
        self.bg_color = float(bg_color)
        self.renderer = FusedRenderer(model, self.H * self.W, iters_per_graph=iters_per_graph, max_steps=max_steps,
                                      dt_gamma=dt_gamma)
        self.dev = self.renderer.dev
        self._intr = (ctypes.c_float * 4)(*[float(v) for v in intrinsics])
        self._aabb = {training: (ctypes.c_float * 6)(*a.detach().cpu().tolist())
                      for training, a in ((True, model.aabb_train), (False, model.aabb_infer))}
        self.rgb8 = torch.zeros(self.H, self.W, 3, dtype=torch.uint8, device=self.dev)
        self.depth8 = torch.zeros(self.H, self.W, dtype=torch.uint8, device=self.dev)
        self.image, self.depth = None, None  # the float results of render(..., floats=True)
        self.loop_image = None  # a model with a background, floats=True: the loop's image before its blend
        self.poses = None
        self._host = None  # frames(): two pinned (rgb, depth) pairs and their events

    def load_weights(self, source=None):
        """source: the weights to render instead of the model's own
        (FusedRenderer.load_weights), e.g. FusedTrainer.ema_params()."""
        self.renderer.load_weights(source)

    def capture(self):
        self.renderer.capture()

    def set_poses(self, poses):
        """The camera path, [n, 4, 4] camera-to-world in ngp coordinates
        (tensor or array): uploaded once, frames index it on the device."""
        poses = poses.detach() if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses, dtype=np.float32))
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] == 0:
            raise ValueError(f"set_poses: poses must be [n, 4, 4] with n >= 1, got {list(poses.shape)}")
        self.poses = poses.to(self.dev, torch.float32).contiguous().clone()

    def __len__(self):
        return 0 if self.poses is None else int(self.poses.shape[0])

    def begin(self, i):
        """The rays of frame i and the loop's initial state into the renderer's
        buffers (one launch; get_rays + near_far_from_aabb + render_init)."""
        if self.poses is None:
            raise RuntimeError("FrameRenderer: set_poses first")
        if not 0 <= i < len(self):
            raise IndexError(f"FrameRenderer: frame {i} of a path of {len(self)}")
        r, m, P = self.renderer, self.model, nat.ptr
        nat.check(nat.lib().ngp_frame_begin(
            P(self.poses), len(self), i, self._intr, self.H, self.W, self._aabb[bool(m.training)],
            float(m.min_near), P(r.rays_o), P(r.rays_d), P(r.nears), P(r.fars), P(r.noises), P(r.alive[0]),
            P(r.rays_t), P(r.weights_sum), P(r.depth), P(r.image), P(r.state), r._stream()), "frame_begin")

    @torch.no_grad()
    def render(self, i, floats=False):
        """Frame i of the path -> device tensors rgb8 [H, W, 3], depth8 [H, W]
        (uint8; this renderer's buffers, overwritten by the next render).
        floats: also keep the float32 colour [H * W, 3] and depth [H * W] the
        bytes were quantised from, in self.image / self.depth."""
        r, lib, P = self.renderer, nat.lib(), nat.ptr
        s = r._stream()
        self.begin(i)
        r.run_loop()
        if floats and self.image is None:
            self.image = torch.zeros(r.N, 3, device=self.dev)
            self.depth = torch.zeros(r.N, device=self.dev)
        bg_color = self.bg_color
        if r._bg:
            # the model's background, blended into the loop's image in place (self.loop_image
            # keeps the image before the blend when floats are asked for); finish then adds 0
            if floats:
                self.loop_image = r.image.clone()
            r.background(blend=True)
            bg_color = 0.0
        nat.check(lib.ngp_frame_finish(self.H, self.W, P(r.image), P(r.weights_sum), P(r.depth), P(r.nears),
                                       P(r.fars), bg_color, P(self.rgb8), P(self.depth8),
                                       P(self.image) if floats else None, P(self.depth) if floats else None, s),
                  "frame_finish")
        return self.rgb8, self.depth8

    def frames(self):
        """Every frame of the path in order as host arrays (rgb [H, W, 3],
        depth [H, W], uint8). The bytes land in one of two alternating pinned
        buffers by a non-blocking copy, and an event says when: the arrays are
        views of that buffer, valid until the generator has been advanced
        twice more, so frame i can be encoded while frame i + 1 renders."""
        if self._host is None:
            self._host = [(torch.empty(self.H, self.W, 3, dtype=torch.uint8).pin_memory(),
                           torch.empty(self.H, self.W, dtype=torch.uint8).pin_memory(),
                           torch.cuda.Event()) for _ in range(2)]
        for i in range(len(self)):
            rgb8, depth8 = self.render(i)
            rgb, depth, ready = self._host[i & 1]
            rgb.copy_(rgb8, non_blocking=True)
            depth.copy_(depth8, non_blocking=True)
            ready.record()
            ready.synchronize()
            yield rgb.numpy(), depth.numpy()


def _save_png(array, path, compress_level):
    from PIL import Image
    Image.fromarray(array).save(path, compress_level=compress_level)
    return path


def write_frames(renderer, out_dir, name, compress_level=1):
    """Render renderer's path and write {name}_{i:04d}_rgb.png and
    {name}_{i:04d}_depth.png (the reference's names, utils.py:785-786) under
    out_dir, RGB and 8-bit grey. The PNGs are encoded by PIL in a pool of 4
    threads (zlib releases the GIL): the two files of frame i are encoded
    while frame i + 1 renders, and are done before frame i + 2 takes their
    pinned buffers. PNG is lossless at every compress_level. -> the paths, in
    frame order, rgb before depth."""
    os.makedirs(out_dir, exist_ok=True)
    paths, pending = [], []
    with ThreadPoolExecutor(max_workers=4) as pool:
        frames = renderer.frames()
        i = 0
        while True:
            if len(pending) == 2:  # frame i - 2 holds the pinned pair frame i is copied into
                for f in pending.pop(0):
                    paths.append(f.result())
            try:
                rgb, depth = next(frames)
            except StopIteration:
                break
            stem = os.path.join(out_dir, f"{name}_{i:04d}")
            pending.append((pool.submit(_save_png, rgb, stem + "_rgb.png", compress_level),
                            pool.submit(_save_png, depth, stem + "_depth.png", compress_level)))
            i += 1
        for pair in pending:
            for f in pair:
                paths.append(f.result())
    return paths


def write_video(renderer, out_dir, name, fps=25, quality=90, png=True):
    """Render renderer's path once and write {name}_rgb.avi and
    {name}_depth.avi under out_dir (the reference's {name}_rgb.mp4 / _depth.mp4,
    utils.py:793-794, as Motion-JPEG in AVI): every frame's rgb8 and depth8 are
    encoded on the device at `quality` (nerf.jpeg.JpegEncoder, 3 components and
    1), and frame i's two files are appended while frame i + 1 renders. png:
    also the PNG sequence, the files write_frames writes for the path; without
    it the uint8 images never leave the device. -> (the two video paths, the
    PNG paths in write_frames' order)."""
    from .jpeg import JpegEncoder
    from .video import AviWriter
    os.makedirs(out_dir, exist_ok=True)
    H, W = renderer.H, renderer.W
    encoders = (JpegEncoder(H, W, 3, quality, renderer.dev), JpegEncoder(H, W, 1, quality, renderer.dev))
    videos = [os.path.join(out_dir, f"{name}_{kind}.avi") for kind in ("rgb", "depth")]
    writers = [AviWriter(p, W, H, fps) for p in videos]

    def rendered():  # frame after frame on the device, and on the host where the PNGs need it
        if png:
            yield from renderer.frames()
        else:
            for i in range(len(renderer)):
                renderer.render(i)
                yield None, None

    paths, pending = [], []
    try:
        with ThreadPoolExecutor(max_workers=4) as pool:
            frames = rendered()
            i = 0
            while True:
                if len(pending) == 2:  # as in write_frames: frame i - 2 holds frame i's pinned pair
                    for f in pending.pop(0):
                        paths.append(f.result())
                try:
                    rgb, depth = next(frames)
                except StopIteration:
                    break
                for enc, image in zip(encoders, (renderer.rgb8, renderer.depth8)):
                    enc.submit(image)
                if i:  # frame i - 1's bytes landed while frame i rendered
                    for enc, w in zip(encoders, writers):
                        w.add(enc.result())
                if png:
                    stem = os.path.join(out_dir, f"{name}_{i:04d}")
                    pending.append((pool.submit(_save_png, rgb, stem + "_rgb.png", 1),
                                    pool.submit(_save_png, depth, stem + "_depth.png", 1)))
                i += 1
            if i:
                for enc, w in zip(encoders, writers):
                    w.add(enc.result())
            for pair in pending:
                for f in pair:
                    paths.append(f.result())
    finally:
        for w in writers:
            w.close()
    return videos, paths
