"""The host side of the test-frame path (nerf/frames.py, nerf/provider.py
interpolate_poses, main_nerf.py's --test flags): no GPU."""
import math
import os

import numpy as np
import pytest
from PIL import Image

import frame_helpers as fh


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _pose(R, t):
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, t
    return P


def _angle(Ra, Rb):
    """The angle of Ra^T Rb from its sine (antisymmetric part) and cosine
    (trace): conditioned well at every angle, unlike acos of the trace near 0.
    The path's float32 entries (2^-24 relative) move it by ~1e-7; the tests allow 1e-5."""
    R = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    s = 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return math.atan2(s, (np.trace(R) - 1) / 2)


# rotations whose quaternion has its largest component in each of w, x, y, z
# (every branch of the matrix -> quaternion conversion), 170 degrees apart at most
POSE_PAIRS = [
    (_pose(_rotation([1, 2, 3], 0.3), [1, 2, 3]), _pose(_rotation([-1, 0.5, 2], 1.9), [-2, 0.5, 1])),
    (_pose(_rotation([1, 0.1, 0], 3.0), [0, 0, 1]), _pose(_rotation([0.1, 1, 0], 2.9), [1, 0, 0])),
    (_pose(_rotation([0, 0.1, 1], 3.1), [0.3, 0.2, 0.1]), _pose(_rotation([0, 0, 1], 0.2), [3, 2, 1])),
    (_pose(np.eye(3), [0, 0, 0]), _pose(_rotation([0, 1, 0], math.radians(170)), [0, 0, 4])),
]


@pytest.mark.parametrize("pair", range(len(POSE_PAIRS)))
@pytest.mark.parametrize("n", [1, 4, 10])
def test_interpolate_poses(pair, n):
    from nerf.provider import interpolate_poses
    p0, p1 = POSE_PAIRS[pair]
    path = interpolate_poses(p0, p1, n)
    assert path.shape == (n + 1, 4, 4) and path.dtype == np.float32
    assert np.abs(path[0] - p0).max() <= 1e-6 and np.abs(path[-1] - p1).max() <= 1e-6
    total = _angle(p0[:3, :3].astype(np.float64), p1[:3, :3].astype(np.float64))
    for i, P in enumerate(path):
        R = P[:3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(R) - 1) <= 1e-5
        assert np.array_equal(P[3], [0, 0, 0, 1])
        # the sine rule: the angle from pose 0 and the translation both sit at ratio_i
        ratio = math.sin((i / n - 0.5) * math.pi) * 0.5 + 0.5
        assert abs(_angle(p0[:3, :3].astype(np.float64), R) - ratio * total) <= 1e-5
        want_t = (1 - ratio) * p0[:3, 3].astype(np.float64) + ratio * p1[:3, 3]
        assert np.abs(P[:3, 3] - want_t).max() <= 1e-6
    if n % 2 == 0:  # the middle pose: half the relative angle, the mid translation
        mid = path[n // 2]
        R = mid[:3, :3].astype(np.float64)
        assert abs(_angle(p0[:3, :3].astype(np.float64), R) - total / 2) <= 1e-5
        assert abs(_angle(R, p1[:3, :3].astype(np.float64)) - total / 2) <= 1e-5
        assert np.abs(mid[:3, 3] - (p0[:3, 3] + p1[:3, 3]) / 2).max() <= 1e-6


def test_interpolate_poses_same_rotation_and_bad_n():
    from nerf.provider import interpolate_poses
    p0, p1 = _pose(_rotation([1, 1, 0], 0.7), [0, 0, 0]), _pose(_rotation([1, 1, 0], 0.7), [2, 0, 0])
    path = interpolate_poses(p0, p1, 2)
    for P in path:
        assert np.abs(P[:3, :3] - p0[:3, :3]).max() <= 1e-6
    assert np.allclose(path[:, 0, 3], [0, 1, 2], atol=1e-6)
    with pytest.raises(ValueError):
        interpolate_poses(p0, p1, 0)


def test_quantisation_rule():
    from nerf.frames import quantise
    x = np.array([np.nan, np.inf, -np.inf, -0.1, -0.0, 0.0, 1.0, 1.0000001, 2.0, 0.5, 1 / 255, 0.999999,
                  np.float32(254) / np.float32(255)], np.float32)
    want = np.array([0, 0, 0, 0, 0, 0, 255, 255, 255, 127, 1, 254, int(np.float32(254) / np.float32(255)
                                                                        * np.float32(255))], np.uint8)
    assert np.array_equal(fh.q(x), want)
    assert np.array_equal(quantise(x), want)
    # on [0, 1] it is the reference's cast; the two statements agree on every kind of input
    rng = np.random.default_rng(0)
    y = rng.uniform(0, 1, 4096).astype(np.float32)
    assert np.array_equal(fh.q(y), (y * 255).astype(np.uint8))
    z = rng.uniform(-0.5, 1.5, (64, 64, 3)).astype(np.float32)
    z[rng.uniform(size=z.shape) < 0.05] = np.nan
    assert np.array_equal(fh.q(z), quantise(z)) and fh.q(z).shape == z.shape


class _Path:
    """What write_frames needs of a renderer: frames() yielding (rgb, depth)."""

    def __init__(self, frames):
        self._frames = frames

    def frames(self):
        # like FrameRenderer.frames(): two alternating buffers, a view valid for two advances
        bufs = [(np.empty((fh.H, fh.W, 3), np.uint8), np.empty((fh.H, fh.W), np.uint8)) for _ in range(2)]
        for i, (rgb, depth) in enumerate(self._frames):
            b = bufs[i & 1]
            b[0][...] = rgb
            b[1][...] = depth
            yield b


def test_write_frames_round_trip(tmp_path):
    from nerf.frames import write_frames
    rng = np.random.default_rng(1)
    frames = [(rng.integers(0, 256, (fh.H, fh.W, 3), dtype=np.uint8), rng.integers(0, 256, (fh.H, fh.W),
                                                                                   dtype=np.uint8))
              for _ in range(5)]
    out = str(tmp_path / "results")
    paths = write_frames(_Path(frames), out, "ngp")
    want = [os.path.join(out, f"ngp_{i:04d}_{kind}.png") for i in range(5) for kind in ("rgb", "depth")]
    assert paths == want and sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in want)
    for i, (rgb, depth) in enumerate(frames):
        a, b = Image.open(want[2 * i]), Image.open(want[2 * i + 1])
        assert a.mode == "RGB" and b.mode == "L" and a.size == (fh.W, fh.H)
        assert np.array_equal(np.asarray(a), rgb) and np.array_equal(np.asarray(b), depth)
    assert write_frames(_Path([]), str(tmp_path / "none"), "ngp") == []


def test_parser_test_flags_and_unchanged_training_defaults():
    import main_nerf
    p = main_nerf.get_parser()
    d = p.parse_args(["scene"])
    assert (d.test, d.ckpt, d.test_frames, d.write_frames) == (False, "latest", 10, False)
    # the training defaults, as before the test flags
    assert (d.iters, d.lr, d.num_rays, d.max_steps, d.update_extra_interval, d.sample_budget) == \
        (30000, 1e-2, 4096, 1024, 16, 2 ** 20)
    assert (d.bound, d.scale, d.dt_gamma, d.min_near, d.density_thresh, d.downscale) == (2, 0.33, 1 / 128, 0.2, 10, 1)
    assert (d.workspace, d.seed, d.save_mesh, d.error_map, d.depth_loss_weight) == ("workspace", 0, False, False, 0.0)
    t = p.parse_args(["scene", "--test", "--ckpt", "a/b.pth", "--test_frames", "24", "--save_mesh"])
    assert (t.test, t.ckpt, t.test_frames, t.save_mesh) == (True, "a/b.pth", 24, True)
    assert p.parse_args(["scene", "--write_frames"]).write_frames


def test_frame_entries_reject_bad_arguments_before_any_device_work():
    """NGP_ERR_ARG for a null or misaligned buffer, an empty or oversized frame
    and a pose index past the stack: found before anything is launched, so the
    pointers here are never dereferenced."""
    import ctypes

    import _ngp_native as nat
    lib = nat.lib()
    intr, aabb = (ctypes.c_float * 4)(40, 40, 16, 12), (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    ptrs = [0x1000 * (k + 1) for k in range(12)]  # poses, 10 ray buffers, state: 16-byte aligned

    def begin(poses=ptrs[0], n_poses=2, index=0, H=24, W=32, bufs=ptrs[1:11], state=ptrs[11]):
        return lib.ngp_frame_begin(poses, n_poses, index, intr, H, W, aabb, 0.2, *bufs, state, None)

    def finish(H=24, W=32, ins=ptrs[:5], rgb8=ptrs[5], depth8=ptrs[6] + 4, image_out=None, depth_out=None):
        return lib.ngp_frame_finish(H, W, *ins, 1.0, rgb8, depth8, image_out, depth_out, None)

    bad = [begin(index=2), begin(H=0), begin(W=0), begin(H=1 << 14, W=1 << 14), begin(poses=None),
           begin(state=None), begin(bufs=ptrs[1:10] + [None]), begin(bufs=[ptrs[1] + 4] + ptrs[2:11]),
           finish(H=0), finish(H=1 << 14, W=1 << 14), finish(ins=[None] + ptrs[1:5]), finish(rgb8=None),
           finish(ins=ptrs[:4] + [ptrs[4] + 8]), finish(rgb8=ptrs[5] + 2), finish(depth8=ptrs[6] + 1),
           finish(image_out=ptrs[7] + 4)]
    assert all(rc != 0 for rc in bad), bad
    assert b"frame_finish" in lib.ngp_last_error()
