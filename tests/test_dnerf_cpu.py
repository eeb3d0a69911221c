"""CPU: the D-NeRF restatements (tests/dnerf_helpers.py) against hand-made
cases, the provider's frame times, the network's state_dict against the
reference's names and shapes, and the front door's rejected options."""
import json
import os

import numpy as np
import pytest
import torch

import dnerf_helpers as dh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- restatements ------------------------------------------------------------------
def test_morton_roundtrip_and_known_codes():
    assert int(dh.morton3(1, 0, 0)) == 1 and int(dh.morton3(0, 1, 0)) == 2 and int(dh.morton3(0, 0, 1)) == 4
    assert int(dh.morton3(3, 5, 6)) == 0b110_101_011  # bit i of x, y, z at 3 i, 3 i + 1, 3 i + 2
    c = np.array([[0, 0, 0], [7, 7, 7], [3, 5, 6], [1023, 0, 512]])
    m = dh.morton3(c[:, 0], c[:, 1], c[:, 2])
    assert m[0] == 0 and m[1] == 511
    assert np.array_equal(dh.morton3_invert(m), c)
    # every cell of an 8^3 cube has its own code below 512
    i = np.arange(8)
    xx, yy, zz = np.meshgrid(i, i, i, indexing="ij")
    assert sorted(dh.morton3(xx.ravel(), yy.ravel(), zz.ravel()).tolist()) == list(range(512))


def test_point_position_hand_cases():
    # H = 2, bound 1: hgs = 0.5, centres at -+0.5; u = 0.5 is the centre, u = 0 the lower face
    p = dh.point_position([[0, 1, 0]], np.array([[0.5, 0.5, 0.0]], np.float32), 0, 2, 1)
    assert np.array_equal(p, np.array([[-0.5, 0.5, -1.0]], np.float32))
    # cascade 1 of bound 2 at H = 8: bound_c = 2, hgs = 0.25, centres (2 c / 7 - 1) * 1.75
    c64, hgs = dh.cell_centre64([[0, 7, 3]], 1, 8, 2)
    assert hgs == 0.25 and np.allclose(c64, [[-1.75, 1.75, -0.25]], atol=1e-15)
    p = dh.point_position([[0, 7, 3]], np.full((1, 3), 0.5, np.float32), 1, 8, 2)
    assert np.abs(p - c64).max() <= 2 ** -22  # the fp32 centre: 6 / 7 through a reciprocal
    # bound 2 clamps nothing at cascade 0 (bound_c = 1); bound 1.5 clamps cascade 1 to 1.5
    assert dh.cascade_scales(0, 8, 2) == (np.float32(0.875), np.float32(0.125))
    assert dh.cascade_scales(1, 8, 1.5) == (np.float32(1.5 - 1.5 / 8), np.float32(1.5 / 8))
    # the jitter spans [-hgs, hgs): every point stays within hgs of its centre
    u = np.random.default_rng(0).random((1000, 3), np.float32)
    cc = np.random.default_rng(1).integers(0, 8, (1000, 3))
    p = dh.point_position(cc, u, 1, 8, 2)
    c64, hgs = dh.cell_centre64(cc, 1, 8, 2)
    assert np.abs(p - c64).max() <= hgs + 2 ** -22


def test_point_time_hand_cases():
    assert dh.point_time([0], 4, [0.5])[0] == np.float32(0.125)
    assert dh.point_time([3], 4, [0.0])[0] == np.float32(0.75)
    assert dh.point_time([1], 2, [0.75])[0] == np.float32(0.875)
    # T = 3: the sum's rounding may step past a slice's end; the restatement keeps it inside
    t = np.repeat(np.arange(3), 1000)
    u = np.tile(np.linspace(0, 1, 1000, endpoint=False), 3).astype(np.float32)
    tm = dh.point_time(t, 3, u)
    lo, hi = dh.slice_bounds32(t, 3)
    assert (tm >= lo).all() and (tm <= hi).all()
    assert np.abs(tm.astype(np.float64) - ((t + 0.5) / 3 + (2 * u.astype(np.float64) - 1) * 0.5 / 3)).max() < 1e-7


def test_ema_pack_ref_hand_case():
    # T = 2, C = 1, 8 cells per slice (H = 2)
    grid = np.array([[[-1, 0, 0.2, 0.8, 1.0, 0.5, 0.0, 2.0]], [[4, 4, 4, 4, 0, 0, 0, 0]]], np.float32)
    tmp = np.array([[[0.5, -1, 0.1, 0.9, -1, 0.5, 0.3, 0.0]], [[-1, -1, -1, -1, -1, -1, -1, 1.0]]], np.float32)
    g, t, total, mean, bits = dh.ema_pack_ref(grid, tmp, 0.5, 0.45)
    want0 = np.array([-1, 0, 0.1, 0.9, 1.0, 0.5, 0.3, 1.0], np.float32)  # max(g / 2, tmp) where both >= 0
    want1 = np.array([4, 4, 4, 4, 0, 0, 0, 1.0], np.float32)
    assert np.array_equal(g[0, 0], want0) and np.array_equal(g[1, 0], want1)
    assert (t == -1).all()
    assert total == pytest.approx(float(want0[1:].astype(np.float64).sum() + want1.astype(np.float64).sum()), rel=1e-15)
    assert mean == np.float32(total / 16)
    # mean = 20.8 / 16 = 1.3 > 0.45: the threshold is 0.45; > is strict
    assert bits.shape == (2, 1)
    assert bits[0, 0] == 0b10111000 and bits[1, 0] == 0b10001111
    # a small global mean wins over density_thresh: slice 1's 4s are above 1.3, slice 0's 1.0 is not
    _, _, _, _, bits = dh.ema_pack_ref(grid, tmp, 0.5, 10.0)
    assert bits[0, 0] == 0 and bits[1, 0] == 0b00001111
    # a value exactly on the threshold is not occupied
    g2 = np.full((1, 1, 8), 0.25, np.float32)
    assert dh.ema_pack_ref(g2, np.full_like(g2, -1), 0.95, 0.25)[4][0, 0] == 0
    # NaN in the grid: NaN mean, every bit clear
    g3 = np.ones((1, 1, 8), np.float32)
    g3[0, 0, 3] = np.nan
    out = dh.ema_pack_ref(g3, np.full_like(g3, -1), 0.95, 0.01)
    assert np.isnan(out[3]) and out[4][0, 0] == 0


def test_encode_ref_hand_case():
    x = np.array([[0.0, 0.5, -2.0]], np.float32)
    e = dh.encode_ref(x, np.array([0.25], np.float32))
    assert e.shape == (1, dh.ENCODE_COLS)
    assert np.array_equal(e[0, :3], [0.0, 0.5, -2.0])
    assert np.allclose(e[0, 3:6], np.sin([0.0, 0.5, -2.0]), atol=1e-16)   # octave 0 sines
    assert np.allclose(e[0, 6:9], np.cos([0.0, 0.5, -2.0]), atol=1e-16)   # octave 0 cosines
    assert np.allclose(e[0, 3 + 6 * 9 + 1], np.sin(0.5 * 512), atol=1e-16)  # octave 9 sine of y
    assert e[0, 63] == 0.25
    assert np.allclose(e[0, 64:66], [np.sin(0.25), np.cos(0.25)], atol=1e-16)
    assert np.allclose(e[0, 74:76], [np.sin(8.0), np.cos(8.0)], atol=1e-16)
    # the repository's plain-torch encoders have the same columns
    tx = dh.torch_encode(torch.from_numpy(x).double(), torch.tensor([[0.25]], dtype=torch.float64)).numpy()
    assert np.abs(tx - e).max() < 1e-15
    # one time for all rows broadcasts
    e2 = dh.encode_ref(np.zeros((3, 3), np.float32), np.array([[1.0]], np.float32))
    assert e2.shape == (3, 76) and (e2[:, 63] == 1.0).all()
    assert dh.half_ulp(1.0) == 2.0 ** -10 and dh.half_ulp(0.75) == 2.0 ** -11 and dh.half_ulp(0.0) == 2.0 ** -24


# ---- provider -----------------------------------------------------------------------
def _three_frames(root, names, times=None):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    frames = []
    for i, name in enumerate(names):
        Image.fromarray(np.full((4, 4, 3), 40 * i, np.uint8)).save(os.path.join(root, name + ".png"))
        fr = {"file_path": "./" + name, "transform_matrix": np.eye(4).tolist()}
        if times is not None:
            fr["time"] = times[i]
        frames.append(fr)
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.7, "frames": frames}, f)
    return root


def test_provider_explicit_times(tmp_path):
    from dnerf import NeRFDataset
    ds = NeRFDataset(_three_frames(str(tmp_path), ["a", "b", "c"], [0.0, 0.25, 1.0]), "cpu", num_rays=8)
    assert ds.times.dtype == torch.float32 and tuple(ds.times.shape) == (3, 1)
    assert ds.times.view(-1).tolist() == [0.0, 0.25, 1.0]  # the largest is 1: left alone
    batch = ds.sample(1)
    assert tuple(batch["time"].shape) == (1, 1) and batch["time"].item() == 0.25
    assert batch["rays_o"].shape == (1, 8, 3) and batch["images"].shape == (1, 8, 3)


def test_provider_times_from_file_names_are_normalised(tmp_path):
    from dnerf import NeRFDataset
    ds = NeRFDataset(_three_frames(str(tmp_path), ["000", "005", "010"]), "cpu", num_rays=8)
    want = np.array([0, 5, 10], np.float32) / (np.float32(10) + np.float32(1e-8))
    assert np.array_equal(ds.times.view(-1).numpy(), want.astype(np.float32))


def test_provider_explicit_times_above_one_are_normalised(tmp_path):
    from dnerf import NeRFDataset, normalize_times
    ds = NeRFDataset(_three_frames(str(tmp_path), ["a", "b", "c"], [0.0, 2.0, 4.0]), "cpu", num_rays=8)
    assert np.allclose(ds.times.view(-1).numpy(), [0.0, 0.5, 1.0], atol=1e-7) and ds.times.max() <= 1
    assert np.array_equal(normalize_times([0.0, 0.5]), np.array([[0.0], [0.5]], np.float32))  # <= 1: left alone


def test_provider_file_names_at_most_one_are_left_alone(tmp_path):
    from dnerf import NeRFDataset
    ds = NeRFDataset(_three_frames(str(tmp_path), ["0", "1", "01"]), "cpu", num_rays=8)
    assert ds.times.view(-1).tolist() == [0.0, 1.0, 1.0]


def test_provider_rejects_a_frame_without_a_time(tmp_path):
    from dnerf import NeRFDataset
    with pytest.raises(ValueError, match="no 'time'"):
        NeRFDataset(_three_frames(str(tmp_path), ["a", "b", "c"]), "cpu")


def test_static_provider_is_unchanged(tmp_path):
    from nerf.provider import NeRFDataset
    ds = NeRFDataset(_three_frames(str(tmp_path), ["a", "b", "c"], [0.0, 0.5, 1.0]), "cpu", num_rays=8)
    assert not hasattr(ds, "times") and "time" not in ds.sample(0)


# ---- network ----------------------------------------------------------------------------
def test_state_dict_has_the_reference_names_and_shapes():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built")
    from dnerf import NeRFNetwork
    with open(os.path.join(ROOT, "tests", "golden", "dnerf_state_dict.json")) as f:
        want = [(name, tuple(shape)) for name, shape in json.load(f)]
    net = NeRFNetwork()
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert sorted(got) == sorted(want)
    assert net.time_size == 64 and net.cascade == 1 and net.grid_size == 128
    assert torch.equal(net.times.view(-1), (torch.arange(64, dtype=torch.float32) + 0.5) / 64)
    # the reference's optimizer groups: grid, sigma, sh, colour, the two frequency encoders, deformation
    groups = net.get_params(1e-2, 1e-3)
    assert [g["lr"] for g in groups] == [1e-2, 1e-3, 1e-2, 1e-3, 1e-2, 1e-2, 1e-3]
    sizes = [sum(p.numel() for p in g["params"]) for g in net.get_params(1e-2, 1e-3)]
    assert sizes == [6119864 * 2, 64 * 108 + 16 * 64, 0, 64 * 31 + 64 * 64 + 3 * 64, 0, 0,
                     128 * 76 + 3 * 128 * 128 + 3 * 128]
    torch.optim.Adam(net.get_params(1e-2, 1e-3), betas=(0.9, 0.99), eps=1e-15)  # empty groups are accepted


def test_small_renderer_shapes_and_cadence():
    from dnerf import NeRFRenderer
    r = NeRFRenderer(bound=2, time_size=3, grid_size=8)
    assert tuple(r.density_grid.shape) == (3, 2, 512) and tuple(r.density_bitfield.shape) == (3, 128)
    assert r.update_chunks() == (False, [(0, 1024), (1024, 2048), (2048, 3072)])
    r.iter_density = 16
    assert r.update_chunks() == (True, [(0, 1024), (1024, 1536)])
    r.iter_density = 100
    assert r.update_chunks() == (False, [])
    assert r.time_slice(torch.tensor([[0.99]])).item() == 2 and r.time_slice(torch.tensor([[1.0]])).item() == 2
    assert r.time_slice(torch.tensor([[0.0]])).item() == 0 and r.time_slice(torch.tensor([[0.34]])).item() == 1
    r.density_grid.fill_(1.0)
    r.reset_extra_state()
    assert r.iter_density == 0 and r.density_grid.abs().sum() == 0
    with pytest.raises(ValueError):
        NeRFRenderer(grid_size=6)
    with pytest.raises(NotImplementedError):
        NeRFRenderer(bg_radius=1.0)


# ---- front door ----------------------------------------------------------------------------
@pytest.mark.parametrize("argv,msg", [(["--basis"], "--basis"), (["--hyper"], "--hyper"), (["--gui"], "--gui"),
                                      (["--bg_radius", "1"], "--bg_radius"), (["--error_map"], "--error_map"),
                                      (["--patch_size", "8"], "--patch_size")])
def test_main_dnerf_rejects_what_is_not_included(argv, msg):
    import main_dnerf
    with pytest.raises(SystemExit) as e:
        main_dnerf.main(["some/scene", "-O"] + argv)
    assert msg in str(e.value) and "not included" in str(e.value)


def test_main_dnerf_takes_the_reference_arguments():
    import main_dnerf
    opt = main_dnerf.get_parser().parse_args(
        "scene -O --test --workspace w --seed 3 --iters 5 --lr 1e-2 --lr_net 1e-3 --ckpt latest --num_rays 64 "
        "--max_steps 128 --update_extra_interval 10 --bound 1 --scale 0.8 --offset 0 0 0 --dt_gamma 0 "
        "--min_near 0.1 --density_thresh 5 --fp16 --preload".split())
    assert opt.update_extra_interval == 10 and opt.lr_net == 1e-3 and opt.preload and opt.fp16
    assert main_dnerf.get_parser().parse_args(["scene"]).update_extra_interval == 100
