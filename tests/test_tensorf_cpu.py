"""CPU: the host side of the TensoRF family (tensoRF/, main_tensoRF.py) and the
references the GPU tests compare against (tests/tensorf_helpers.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tensorf_helpers as th
from tensoRF import network as tn
from tensoRF.vm import line_from_ref, line_to_ref, plane_from_ref, plane_to_ref, vm_quantum, vm_reference


# ---- the numpy restatement against torch's grid_sample, in float64 ---------------------------

@pytest.mark.parametrize("res", [(5, 3, 2), (2, 2, 2), (7, 4, 9)])
@pytest.mark.parametrize("ranks", [(16, 16, 16), (1, 1, 1), (4, 8, 12)])
def test_numpy_restatement_equals_vm_reference(res, ranks):
    planes, lines = th.make_set(res, ranks, seed=1)
    c, first_out, n_out = th.normalised_points(res, 600, seed=2)
    p64, l64 = [p.double() for p in planes], [v.double() for v in lines]
    for aabb in (None, th.SHRUNK_BOX):
        x = c if aabb is None else th.world_points(c, aabb).astype(np.float64)
        box = None if aabb is None else torch.tensor(aabb, dtype=torch.float64)
        for mode in ("sum", "concat"):
            ref = vm_reference(torch.from_numpy(x), p64, l64, mode, aabb=box).numpy()
            got = th.vm_numpy(x, planes, lines, mode, aabb=aabb)
            assert ref.shape == got.shape == ((600,) if mode == "sum" else (600, sum(ranks)))
            # the same formula in another association: a few float64 ulps of values below 1
            assert np.abs(ref - got).max() <= 1e-15, (mode, aabb)
            assert not np.isnan(ref).any()
            if aabb is None:  # wholly outside: exactly zero
                assert np.all(ref[first_out:first_out + n_out] == 0)
                assert np.all(got[first_out:first_out + n_out] == 0)


def test_sampling_semantics_at_the_edges():
    """1 + eps keeps weight 1 - eps (res - 1) / 2 of the last texel; a line is
    plain linear interpolation over D; resolution 2 gives no NaN."""
    res = (5, 3, 2)
    planes = [torch.ones(1, 1, res[m1], res[m0], dtype=torch.float64) for m0, m1 in th.MAT_IDS]
    lines = [torch.ones(1, 1, res[v], 1, dtype=torch.float64) for v in th.VEC_IDS]
    eps = 1e-6
    x = torch.tensor([[1 + eps, 0.0, 0.0]], dtype=torch.float64)
    prod = vm_reference(x, planes, lines, "concat")[0]
    w = 1 - eps * (res[0] - 1) / 2
    assert abs(prod[0] - w) < 1e-12 and abs(prod[1] - w) < 1e-12 and abs(prod[2] - w) < 1e-12
    ramp = torch.arange(5, dtype=torch.float64).view(1, 1, 5, 1)
    lines[2] = ramp  # the line over axis 0
    x = torch.tensor([[-1.0, 0, 0], [-0.25, 0, 0], [1.0, 0, 0]], dtype=torch.float64)
    assert torch.allclose(vm_reference(x, planes, lines, "concat")[:, 2],
                          torch.tensor([0.0, 1.5, 4.0], dtype=torch.float64), atol=1e-14)


def test_layout_conversions_round_trip():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(1, 7, 5, 3, generator=g)
    v = torch.randn(1, 7, 6, 1, generator=g)
    q, w = plane_from_ref(p), line_from_ref(v)
    assert q.shape == (5, 3, 7) and w.shape == (6, 7) and q.is_contiguous() and w.is_contiguous()
    assert q[4, 2, 6] == p[0, 6, 4, 2] and w[5, 3] == v[0, 3, 5, 0]
    assert torch.equal(plane_to_ref(q), p) and torch.equal(line_to_ref(w), v)
    assert plane_to_ref(q).is_contiguous() and line_to_ref(w).is_contiguous()


def test_quantum_is_a_power_of_two_above_the_largest_gradient():
    assert vm_quantum(torch.tensor([0.0, 0.0])) == 0.0
    assert vm_quantum(torch.tensor([0.5, -1.0])) == 2.0 ** (1 - 32)      # 2^1 > 1
    assert vm_quantum(torch.tensor([0.75]), torch.tensor([-0.3])) == 2.0 ** (0 - 32)
    assert vm_quantum(None, torch.tensor([65536.0 * 3])) == 2.0 ** (18 - 32)


# ---- the model's host side ------------------------------------------------------------------

def _model(res=(5, 3, 2), **kw):
    torch.manual_seed(0)
    return tn.NeRFNetwork(resolution=res, sigma_rank=(2, 3, 4), color_rank=(3, 3, 3), **kw)


def test_defaults_and_parameter_shapes():
    import inspect
    sig = inspect.signature(tn.NeRFNetwork.__init__).parameters
    assert list(sig["resolution"].default) == [128] * 3 and list(sig["sigma_rank"].default) == [16] * 3
    assert list(sig["color_rank"].default) == [48] * 3 and sig["color_feat_dim"].default == 27
    assert sig["num_layers"].default == 3 and sig["hidden_dim"].default == 128
    m = _model()
    assert [tuple(p.shape) for p in m.sigma_mat] == [(3, 5, 2), (2, 5, 3), (2, 3, 4)]  # [H, W, R]
    assert [tuple(p.shape) for p in m.sigma_vec] == [(2, 2), (3, 3), (5, 4)]  # [D, R]
    assert m.basis_mat.weight.shape == (27, 9) and m.basis_mat.bias is None
    assert [tuple(l.weight.shape) for l in m.color_net] == [(128, 27 * 5 + 15), (128, 128), (3, 128)]
    assert all(l.bias is None for l in m.color_net)
    groups = m.get_params(2e-2, 1e-3)
    assert [g["lr"] for g in groups] == [2e-2] * 4 + [1e-3] * 2
    assert sum(len(g["params"]) for g in groups) == len(list(m.parameters()))
    with pytest.raises(NotImplementedError):
        _model(bg_radius=1.0)


def test_state_dict_speaks_the_reference_layout():
    m = _model()
    sd = m.state_dict()
    assert sd["sigma_mat.1"].shape == (1, 3, 2, 5) and sd["color_vec.2"].shape == (1, 3, 5, 1)
    assert torch.equal(sd["sigma_mat.1"], plane_to_ref(m.sigma_mat[1].data))
    assert m.sigma_mat[1].shape == (2, 5, 3)  # the model keeps its own layout
    # a reference-layout state of another resolution loads into a fresh model
    big = _model(res=(4, 6, 3))
    with torch.no_grad():
        for p in big.parameters():
            p.normal_()
    big.aabb_train.copy_(torch.tensor(th.SHRUNK_BOX))
    m.load_state_dict(big.state_dict())
    assert m.resolution == [4, 6, 3] and torch.equal(m.aabb_train, big.aabb_train)
    for a, b in zip(m.parameters(), big.parameters()):
        assert torch.equal(a, b)
    assert m.density_loss().item() == pytest.approx(
        sum(p.abs().mean().item() for p in list(big.sigma_mat) + list(big.sigma_vec)), rel=1e-6)


def test_upsample_model_equals_interpolate_on_the_reference_layout():
    m = _model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    new = [7, 4, 6]
    m.upsample_model(new)
    assert m.resolution == new
    after = m.state_dict()
    for name in ("sigma", "color"):
        for i, (m0, m1) in enumerate(th.MAT_IDS):
            want = F.interpolate(before[f"{name}_mat.{i}"], size=(new[m1], new[m0]), mode="bilinear",
                                 align_corners=True)
            assert torch.equal(after[f"{name}_mat.{i}"], want)
            want = F.interpolate(before[f"{name}_vec.{i}"], size=(new[th.VEC_IDS[i]], 1), mode="bilinear",
                                 align_corners=True)
            assert torch.equal(after[f"{name}_vec.{i}"], want)
    assert all(p.is_contiguous() and p.requires_grad for p in m.parameters())


def test_morton_invert_matches_the_provider_codes():
    from nerf.provider import _morton3
    rng = np.random.default_rng(0)
    xyz = rng.integers(0, 1024, (500, 3))
    codes = torch.from_numpy(_morton3(xyz[:, 0], xyz[:, 1], xyz[:, 2]))
    assert np.array_equal(tn.morton3D_invert(codes).numpy(), xyz)


def test_shrink_model_on_a_hand_made_grid():
    """grid_size 8, bound 1, resolution (8, 16, 4): cells x 2..5, y 4..7, z 0..3
    occupied. Their centres lie at (2 c / 7 - 1) * 0.875, the box is grown by
    1 / 8: lo = (-0.5, 0, -1), hi = (0.5, 1, 0), which are the cells' outer
    faces here. In texels of 2 / resolution that is the slice [2, 6) x [8, 16)
    x [0, 2)."""
    from nerf.provider import _morton3
    torch.manual_seed(0)
    m = tn.NeRFNetwork(resolution=(8, 16, 4), sigma_rank=(2, 2, 2), color_rank=(3, 3, 3), bound=1, cuda_ray=True,
                       grid_size=8, density_thresh=10)
    xs, ys, zs = np.meshgrid(np.arange(2, 6), np.arange(4, 8), np.arange(0, 4), indexing="ij")
    m.density_grid[0, torch.from_numpy(_morton3(xs.reshape(-1), ys.reshape(-1), zs.reshape(-1)))] = 5.0
    m.mean_density = 1.0  # threshold min(10, 1)
    centre = lambda c: (2 * c / 7 - 1) * 0.875
    lo = np.array([centre(2), centre(4), centre(0)]) - 0.125
    hi = np.array([centre(5), centre(7), centre(3)]) + 0.125
    units = 2.0 / np.array([8, 16, 4])
    tl = np.clip(np.round((lo + 1) / units), 0, None).astype(int)
    br = np.minimum(np.round((hi + 1) / units), [8, 16, 4]).astype(int)
    assert tl.tolist() == [2, 8, 0] and br.tolist() == [6, 16, 2]
    old = {k: v.clone() for k, v in m.state_dict().items()}
    got = m.shrink_model()
    assert got == (tl.tolist(), br.tolist())
    assert np.allclose(m.aabb_train.numpy(), np.concatenate([lo, hi]), atol=1e-6)
    assert m.resolution == [4, 8, 2]
    new = m.state_dict()
    for name in ("sigma", "color"):
        for i, (m0, m1) in enumerate(th.MAT_IDS):
            v = th.VEC_IDS[i]
            assert torch.equal(new[f"{name}_mat.{i}"], old[f"{name}_mat.{i}"][..., tl[m1]:br[m1], tl[m0]:br[m0]])
            assert torch.equal(new[f"{name}_vec.{i}"], old[f"{name}_vec.{i}"][..., tl[v]:br[v], :])
    assert torch.equal(new["aabb_infer"], old["aabb_infer"])
    # an empty grid changes nothing
    m.density_grid.zero_()
    assert m.shrink_model() is None and m.resolution == [4, 8, 2]


def test_upsample_resolution_arithmetic():
    # the reference's defaults: five steps from 128 to 300
    assert tn.upsample_schedule(128, 300, 5) == [152, 180, 213, 253, 300]
    assert tn.upsample_schedule(16, 24, 1) == [24]
    # a cube keeps the budget's edge (up to the truncation of a float32 quotient)
    assert tn.upsample_resolution([-1, -1, -1, 1, 1, 1], 24 ** 3) in ([24, 24, 24], [23, 23, 23])
    # a 2 : 1 : 1 box of 2 * 16^3 voxels: the edge is 1 / 8, so 32 x 16 x 16 up to the truncation
    reso = tn.upsample_resolution([-2, -1, -1, 2, 1, 1], 2 * 16 ** 3)
    assert reso[0] in (31, 32) and reso[1] == reso[2] and reso[1] in (15, 16)
    aabb = np.array([-0.5, 0.0, -1.0, 0.5, 1.0, 0.5], np.float32)
    ext = aabb[3:] - aabb[:3]
    vox = np.cbrt(np.prod(ext) / np.float32(100 ** 3))
    assert tn.upsample_resolution(aabb, 100 ** 3) == (ext / vox).astype(np.int32).tolist() == [87, 87, 131]


def test_argparse_defaults():
    import main_tensoRF
    opt = main_tensoRF.get_parser().parse_args(["scene"])
    assert opt.path == "scene" and not opt.O and not opt.test and opt.workspace == "workspace" and opt.seed == 0
    assert opt.iters == 30000 and opt.lr0 == 2e-2 and opt.lr1 == 1e-3 and opt.num_rays == 4096
    assert opt.max_steps == 1024 and opt.update_extra_interval == 16 and opt.l1_reg_weight == 1e-4
    assert opt.resolution0 == 128 and opt.resolution1 == 300
    assert opt.upsample_model_steps == [2000, 3000, 4000, 5500, 7000]
    assert opt.bound == 2 and opt.scale == 0.33 and opt.offset == [0, 0, 0] and opt.dt_gamma == 1 / 128
    assert opt.min_near == 0.2 and opt.density_thresh == 10 and opt.downscale == 1 and opt.bg_radius == -1
    # nargs='*' replaces the default instead of appending to it
    opt = main_tensoRF.get_parser().parse_args(["scene", "--upsample_model_steps", "100", "200"])
    assert opt.upsample_model_steps == [100, 200]
    with pytest.raises(SystemExit):
        main_tensoRF.main(["scene", "--bg_radius", "2"])
