"""GPU: the TensoRF family (csrc/tensorf.hip, tensoRF/, main_tensoRF.py).

The kernels are compared with vm_reference (torch's grid_sample) in float64,
which tests/test_tensorf_cpu.py holds to a numpy restatement. Every tolerance
is 4 x the largest error of vm_reference in float32 on the CPU against float64
on the same inputs (room for another summation order and for fma contraction,
nothing more); the backward adds the fixed-point quantum times the number of
points, the most contributions one entry can take."""
import os

import pytest
import torch
import torch.nn.functional as F

import tensorf_helpers as th
from tensoRF import NeRFNetwork, TensoRFTrainer, vm_quantum, vm_reference, vm_sample

pytestmark = pytest.mark.gpu

N_FULL = 4097
SIZES = (1, 63, 64, 65, N_FULL)
_CASES = {}


def case(res, ranks, aabb):
    """One configuration's inputs and float64 references on N_FULL points, computed once."""
    key = (res, ranks, aabb)
    if key not in _CASES:
        planes, lines = th.make_set(res, ranks, seed=3)
        c, first_out, n_out = th.normalised_points(res, N_FULL, seed=4)
        x = th.world_points(c, aabb)
        ref = {mode: th.reference_error(x, planes, lines, mode, aabb) for mode in ("sum", "concat")}
        _CASES[key] = dict(planes=planes, lines=lines, x=x, ref=ref,
                           outside=slice(first_out, first_out + n_out) if aabb == th.UNIT_BOX else None)
    return _CASES[key]


# ---- forward -------------------------------------------------------------------------------

FORWARD = [(res, ranks, th.UNIT_BOX) for res in ((5, 3, 2), (2, 2, 2))
           for ranks in ((16, 16, 16), (1, 1, 1), (4, 8, 12), (48, 48, 48))]
FORWARD += [((5, 3, 2), (4, 8, 12), th.SHRUNK_BOX), ((5, 3, 2), (16, 16, 16), th.SHRUNK_BOX)]


@pytest.mark.parametrize("res,ranks,aabb", FORWARD)
def test_forward_against_float64(cuda, res, ranks, aabb):
    """Both modes, every N of SIZES (prefixes of one point set: the box
    corners, the lattice nodes, 1 + 1e-6 / -1.5 / 2.0 on each axis, points
    outside, uniform points in [-1.2, 1.2]^3). Measured on an MI355X: see
    DESIGN.md section 22."""
    cs = case(res, ranks, aabb)
    planes, lines = th.to_param_layout(cs["planes"], cs["lines"], cuda)
    box = torch.tensor(aabb, device=cuda)
    for n in SIZES:
        x = torch.from_numpy(cs["x"][:n]).to(cuda)
        both = vm_sample(x, box, (planes, lines), (planes, lines))
        alone = (vm_sample(x, box, sigma=(planes, lines))[0], vm_sample(x, box, color=(planes, lines))[1])
        for mode, got, got1 in (("sum", both[0], alone[0]), ("concat", both[1], alone[1])):
            base, ref64 = cs["ref"][mode]
            assert torch.equal(got, got1)  # one call for two sets = two calls
            err = float((got.double().cpu() - ref64[:n]).abs().max())
            print(f"res {res} ranks {ranks} n={n} {mode}: max error {err:.3e}, float32 reference {base:.3e}")
            assert got.shape == ref64[:n].shape and got.dtype == torch.float32
            assert err <= 4 * base
            if cs["outside"] is not None and n == N_FULL:
                assert torch.all(got[cs["outside"]] == 0)
                assert torch.all(ref64[cs["outside"]] == 0)


def test_forward_empty_and_argument_checks(cuda):
    cs = case((5, 3, 2), (4, 8, 12), th.UNIT_BOX)
    planes, lines = th.to_param_layout(cs["planes"], cs["lines"], cuda)
    box = torch.tensor(th.UNIT_BOX, device=cuda)
    s, p = vm_sample(torch.empty(0, 3, device=cuda), box, (planes, lines), (planes, lines))
    assert s.shape == (0,) and p.shape == (0, 24)
    with pytest.raises(ValueError):
        vm_sample(torch.zeros(1, 3, device=cuda), box)
    with pytest.raises(RuntimeError, match="texels"):
        vm_sample(torch.zeros(1, 3, device=cuda), box, (planes, [lines[0], lines[1], lines[2][:3].contiguous()]))
    with pytest.raises(RuntimeError, match="CUDA"):
        vm_sample(torch.zeros(1, 3), box, (planes, lines))


# ---- backward ------------------------------------------------------------------------------

def _reference_grads(x, planes, lines_, g_sigma, g_prod, aabb, dtype):
    """Autograd of vm_reference on the CPU in `dtype` -> gradients in the parameter layout
    [sum planes, sum lines, cat planes, cat lines] (float64)."""
    from tensoRF.vm import line_from_ref, plane_from_ref
    box = torch.tensor(aabb, dtype=dtype)
    out = []
    for mode, g in (("sum", g_sigma), ("concat", g_prod)):
        if g is None:
            continue
        ps = [p.to(dtype).requires_grad_() for p in planes[mode]]
        ls = [v.to(dtype).requires_grad_() for v in lines_[mode]]
        vm_reference(torch.as_tensor(x).to(dtype), ps, ls, mode, aabb=box).backward(g.to(dtype))
        out += [plane_from_ref(p.grad).double() for p in ps] + [line_from_ref(v.grad).double() for v in ls]
    return out


def _kernel_grads(cuda, x, planes, lines_, g_sigma, g_prod, aabb):
    sets, leaves = {}, []
    for mode, g in (("sum", g_sigma), ("concat", g_prod)):
        if g is None:
            sets[mode] = None
            continue
        ps, ls = th.to_param_layout(planes[mode], lines_[mode], cuda)
        ps, ls = [p.requires_grad_() for p in ps], [v.requires_grad_() for v in ls]
        sets[mode] = (ps, ls)
        leaves += ps + ls
    s, p = vm_sample(torch.as_tensor(x).to(cuda), torch.tensor(aabb, device=cuda), sets["sum"], sets["concat"])
    outs, gs = [], []
    if g_sigma is not None:
        outs.append(s), gs.append(g_sigma.to(cuda))
    if g_prod is not None:
        outs.append(p), gs.append(g_prod.to(cuda))
    return torch.autograd.grad(outs, leaves, gs)


@pytest.mark.parametrize("which", ["both", "sum", "concat"])
def test_backward_exact_sums(cuda, which):
    """4097 points on the corners of a (2, 2, 2) texture (all weights 0 or 1),
    integer parameters in [-3, 3], gradients 2^-3 .. 2^3: every contribution
    collides and every sum is exact in float32, so the plane and line gradients
    equal the float64 reference exactly. A lost update or a wrong reduction
    fails here."""
    g = torch.Generator().manual_seed(5)
    res, n = (2, 2, 2), N_FULL
    planes = {"sum": None, "concat": None}
    lines_ = {"sum": None, "concat": None}
    planes["sum"], lines_["sum"] = th.make_set(res, (16, 16, 16), seed=6, integers=True)
    planes["concat"], lines_["concat"] = th.make_set(res, (4, 8, 12), seed=7, integers=True)
    x = (torch.randint(0, 2, (n, 3), generator=g) * 2 - 1).float().numpy()
    g_sigma = 2.0 ** torch.randint(-3, 4, (n,), generator=g).float() if which in ("both", "sum") else None
    g_prod = 2.0 ** torch.randint(-3, 4, (n, 24), generator=g).float() if which in ("both", "concat") else None
    want = _reference_grads(x, planes, lines_, g_sigma, g_prod, th.UNIT_BOX, torch.float64)
    got = _kernel_grads(cuda, x, planes, lines_, g_sigma, g_prod, th.UNIT_BOX)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == torch.float32
        assert b.abs().max() > 16, "the sums must be large enough to collide"
        assert torch.equal(a.double().cpu(), b), f"gradient {k}"


BACKWARD = [((5, 3, 2), (16, 16, 16), (48, 48, 48), th.UNIT_BOX, N_FULL),
            ((5, 3, 2), (4, 8, 12), (1, 1, 1), th.SHRUNK_BOX, N_FULL),
            ((2, 2, 2), (1, 1, 1), (16, 16, 16), th.UNIT_BOX, 65),
            # a line of more than 512 texels is summed in global memory, the others in LDS
            ((513, 3, 2), (4, 8, 12), (16, 16, 16), th.UNIT_BOX, 2049)]


@pytest.mark.parametrize("res,sum_ranks,cat_ranks,aabb,n", BACKWARD)
def test_backward_against_float64(cuda, res, sum_ranks, cat_ranks, aabb, n):
    """Against float64 autograd of vm_reference on the forward's inputs, with
    output gradients of GradScaler size (65536 x N(0, 1) / n). Tolerance per
    tensor: 4 x the float32 CPU autograd's error + n quanta. Two runs give the
    same bits."""
    gen = torch.Generator().manual_seed(8)
    planes = {"sum": None, "concat": None}
    lines_ = {"sum": None, "concat": None}
    planes["sum"], lines_["sum"] = th.make_set(res, sum_ranks, seed=9)
    planes["concat"], lines_["concat"] = th.make_set(res, cat_ranks, seed=10)
    c, _, _ = th.normalised_points(res, max(n, 80), seed=11)
    x = th.world_points(c, aabb)[-n:] if n < 80 else th.world_points(c, aabb)
    g_sigma = 65536.0 / n * torch.randn(n, generator=gen)
    g_prod = 65536.0 / n * torch.randn(n, sum(cat_ranks), generator=gen)
    want = _reference_grads(x, planes, lines_, g_sigma, g_prod, aabb, torch.float64)
    ref32 = _reference_grads(x, planes, lines_, g_sigma, g_prod, aabb, torch.float32)
    got = _kernel_grads(cuda, x, planes, lines_, g_sigma, g_prod, aabb)
    again = _kernel_grads(cuda, x, planes, lines_, g_sigma, g_prod, aabb)
    quantum = vm_quantum(g_sigma, g_prod)
    assert 0 < quantum <= 2.0 ** -32 * 2 * max(float(g_sigma.abs().max()), float(g_prod.abs().max()))
    for k, (a, a2, b, b32) in enumerate(zip(got, again, want, ref32)):
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32)), f"gradient {k}: two runs differ"
        base = float((b32 - b).abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"res {res} gradient {k} {tuple(a.shape)}: max error {err:.3e}, float32 reference {base:.3e}, "
              f"n quanta {n * quantum:.3e}, max |g| {float(b.abs().max()):.3e}")
        assert err <= 4 * base + n * quantum, f"gradient {k}"


def test_backward_special_gradients(cuda):
    """No gradient with respect to x; an unused output gives zero gradients
    for its set; zero gradients give zeros; a gradient that is not finite makes
    every value NaN (the GradScaler then skips the step)."""
    cs = case((5, 3, 2), (4, 8, 12), th.UNIT_BOX)
    box = torch.tensor(th.UNIT_BOX, device=cuda)

    def leaves():
        ps, ls = th.to_param_layout(cs["planes"], cs["lines"], cuda)
        return [p.requires_grad_() for p in ps], [v.requires_grad_() for v in ls]

    x = torch.from_numpy(cs["x"][:65]).to(cuda)
    ps, ls = leaves()
    with pytest.raises(RuntimeError, match="no gradient with respect to x"):
        s, _ = vm_sample(x.clone().requires_grad_(), box, (ps, ls))
        s.sum().backward()
    ps, ls = leaves()
    qs, ms = leaves()
    s, p = vm_sample(x, box, (ps, ls), (qs, ms))
    s.sum().backward()  # the products are not used
    assert all(t.grad.abs().sum() > 0 for t in ps + ls) and all(torch.all(t.grad == 0) for t in qs + ms)
    ps, ls = leaves()
    s, _ = vm_sample(x, box, (ps, ls))
    (s * 0).sum().backward()
    assert all(torch.all(t.grad == 0) for t in ps + ls)
    ps, ls = leaves()
    s, _ = vm_sample(x, box, (ps, ls))
    g = torch.ones_like(s)
    g[7] = float("inf")
    s.backward(g)
    assert all(torch.isnan(t.grad).all() for t in ps + ls)


# ---- the network ---------------------------------------------------------------------------

def _torch_network(model, x, d, dtype):
    """The model from its reference-layout state_dict in plain torch: vm_reference, Linear layers,
    torch's exp and sigmoid. The frequency encodings are the model's own (tests/test_gpu_freq.py)."""
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in model.state_dict().items()}
    smat, svec = [sd[f"sigma_mat.{i}"] for i in range(3)], [sd[f"sigma_vec.{i}"] for i in range(3)]
    cmat, cvec = [sd[f"color_mat.{i}"] for i in range(3)], [sd[f"color_vec.{i}"] for i in range(3)]
    x = x.to(dtype)
    sigma = torch.exp(vm_reference(x, smat, svec, "sum", aabb=sd["aabb_train"]))
    feat = vm_reference(x, cmat, cvec, "concat", aabb=sd["aabb_train"]) @ sd["basis_mat.weight"].t()
    h = torch.cat([model.encoder(feat.float()).to(dtype), model.encoder_dir(d).to(dtype)], -1)
    for l in range(3):
        h = h @ sd[f"color_net.{l}.weight"].t()
        if l != 2:
            h = torch.relu(h)
    return sigma, torch.sigmoid(h)


def test_network_against_plain_torch(cuda):
    """forward, density and color(mask) at fp32 without autocast against the
    plain-torch network in float64; tolerance 4 x the plain-torch network's own
    float32 error on these inputs. density_loss equals the torch expression."""
    torch.manual_seed(0)
    model = NeRFNetwork(resolution=(9, 7, 5), sigma_rank=(16, 16, 16), color_rank=(48, 48, 48), bound=1).to(cuda)
    model.aabb_train.copy_(torch.tensor(th.SHRUNK_BOX, device=cuda))
    n = 1000
    x = (torch.rand(n, 3, device=cuda) * 2 - 1) * 1.05
    d = F.normalize(torch.randn(n, 3, device=cuda), dim=-1)
    with torch.no_grad():
        s64, c64 = _torch_network(model, x, d, torch.float64)
        s32, c32 = _torch_network(model, x, d, torch.float32)
        sigma, rgb = model(x, d)
        dens = model.density(x)["sigma"]
        mask = torch.rand(n, device=cuda) < 0.3
        masked = model.color(x, d, mask=mask)
        unmasked = model.color(x, d)
        empty = model.color(x, d, mask=torch.zeros(n, dtype=torch.bool, device=cuda))
    tol_s = 4 * float(((s32.double() - s64).abs() / s64).max())
    tol_c = 4 * float((c32.double() - c64).abs().max())
    err_s = float(((sigma.double() - s64).abs() / s64).max())
    err_c = float((rgb.double() - c64).abs().max())
    print(f"sigma: relative error {err_s:.3e} (bound {tol_s:.3e}); rgb: error {err_c:.3e} (bound {tol_c:.3e})")
    assert sigma.shape == (n,) and rgb.shape == (n, 3)
    assert err_s <= tol_s and err_c <= tol_c
    assert torch.equal(dens, sigma) and torch.equal(unmasked, rgb)
    assert torch.all(masked[~mask] == 0) and masked.shape == (n, 3)
    assert float((masked[mask].double() - c64[mask]).abs().max()) <= tol_c
    assert empty.shape == (n, 3) and torch.all(empty == 0)
    want = sum(p.abs().mean() for p in list(model.sigma_mat) + list(model.sigma_vec))
    assert torch.allclose(model.density_loss(), want, rtol=1e-6, atol=0)


# ---- training ------------------------------------------------------------------------------

def test_training_upsamples_and_learns(cuda, tmp_path):
    """200 steps on the 6-view 32 x 32 Lego scene of the image-training tests,
    resolution 16, one upsample towards 24 at step 100."""
    from nerf.provider import NeRFDataset
    from test_gpu_fused_images import _write_scene
    scene = _write_scene(str(tmp_path), 6, 32, 32)
    data = NeRFDataset(scene, cuda, type="train", scale=1.0, num_rays=1024, store="uint8")
    torch.manual_seed(0)

    def fresh():
        return NeRFNetwork(resolution=[16] * 3, sigma_rank=[8] * 3, color_rank=[12] * 3, bound=1, cuda_ray=True,
                           density_thresh=10, min_near=0.2).to(cuda)

    model = fresh()
    model.train()
    tr = TensoRFTrainer(model, data, workspace=str(tmp_path / "ws"), iters=200, upsample_model_steps=[100],
                        upsample_resolutions=[24], max_steps=256, log=None)
    shapes0 = [tuple(p.shape) for p in model.parameters()]
    opt0 = tr.optimizer
    losses = []
    for step in range(200):
        losses.append(tr.train_step())
        if step == 98:
            assert any(len(s) > 0 for s in tr.optimizer.state.values())  # Adam has state before the upsample
        if step == 99:  # the upsample ran at the end of step 100
            assert tr.upsamples_done == 1 and tr.optimizer is not opt0 and len(tr.optimizer.state) == 0
            assert tr.optimizer.param_groups[0]["lr"] == 2e-2  # the schedule starts over
    losses = torch.stack(losses).float().cpu()
    assert torch.isfinite(losses).all()
    shapes1 = [tuple(p.shape) for p in model.parameters()]
    assert shapes1[:12] != shapes0[:12] and shapes1[12:] == shapes0[12:]  # the planes and lines changed, the MLP not
    assert model.resolution != [16] * 3 and min(model.resolution) >= 2
    params = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    assert params == {id(p) for p in model.parameters()} and len(tr.optimizer.state) > 0
    first, last = float(losses[:20].mean()), float(losses[-20:].mean())
    print(f"mean loss of the first 20 steps {first:.5f}, of the last 20 {last:.5f}; resolution {model.resolution}")
    assert last < first
    # a checkpoint saved after the upsample loads into a fresh resolution-16 model
    path = tr.save_checkpoint()
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["resolution"] == model.resolution and torch.equal(ck["aabb_train"], model.aabb_train.cpu())
    assert ck["model"]["sigma_mat.0"].dim() == 4  # the reference's layout
    pts = torch.rand(4096, 3, device=cuda) * 2 - 1
    model2 = fresh()
    tr2 = TensoRFTrainer(model2, data, workspace=str(tmp_path / "ws"), iters=200, upsample_model_steps=[100],
                         upsample_resolutions=[24], max_steps=256, log=None)
    tr2.load_checkpoint()
    assert model2.resolution == model.resolution and tr2.global_step == 200 and tr2.upsamples_done == 1
    with torch.no_grad():
        a, b = model.density(pts)["sigma"], model2.density(pts)["sigma"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert os.path.exists(path)
