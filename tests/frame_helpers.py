"""Shared by the frame tests (test_frames_cpu.py, test_gpu_frames.py): a numpy
statement of the frame quantisation and the shape the GPU tests render at."""
import numpy as np

# non-square (a row / column swap shows), H * W = 1961 odd: a tail of one pixel
# after the 4-pixel groups and a partial second workgroup of 1024 pixels
H, W = 37, 53


def q(x):
    """q(x) = uint8(clamp(x, 0, 1) * 255), truncating; 0 for a non-finite x:
    the reference's (x * 255).astype(np.uint8) (nerf/utils.py:776, :779) made
    total. Written apart from nerf.frames.quantise on purpose."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.uint8)
    fin = np.isfinite(x)
    v = np.minimum(np.maximum(x[fin], np.float32(0)), np.float32(1)) * np.float32(255)
    out[fin] = np.floor(v).astype(np.uint8)
    return out


def scaled_intrinsics(data, h=H, w=W):
    """data's camera at h x w pixels (as tests/test_gpu_render.py::_rays scales it)."""
    return data.intrinsics * np.array([w / data.W, h / data.H, w / data.W, h / data.H], np.float32)
