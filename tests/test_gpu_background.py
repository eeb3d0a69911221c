"""GPU: the background model on the fused engine (the reference's --bg_radius;
csrc/background.hip): the forward against a float64
restatement and the autograd ops, the step against autograd, off = unchanged,
graph = eager, the found-inf flag, that it learns a backdrop, frames and the
command line, the checkpoint round trip.

The backward's cross-wave sums are integer (fixed-point) atomics, so a run
with the model on is bit-reproducible: the comparisons between runs are
bitwise."""
import copy

import numpy as np
import pytest
import torch

import background_helpers as bh
from depth_helpers import write_scene

pytestmark = pytest.mark.gpu

N_RAYS = 1024
M_ROWS = 30000 + 128 - 30000 % 128


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    def make(name, fn, *args, **kw):
        return fn(str(tmp_path_factory.mktemp(name)), *args, **kw)
    return {"rgba32": make("rgba32", write_scene, 6, 32, 32, depth=False),
            "sky64": make("sky64", bh.write_backdrop_scene, 8, 64, 64, heldout=1)}


def _dataset(path, dev, store="uint8", type="train", scale=1.0, **kw):
    from nerf.provider import NeRFDataset
    return NeRFDataset(path, dev, type=type, scale=scale, num_rays=N_RAYS, store=store, **kw)


def _model(dev, bound=1, bits=None, bg_radius=4, **kw):
    """A non-trivial field: table values larger than the 1e-4 init, in both
    tables (N(0, 0.05) and, for the background's, N(0, 0.3): its 8 features then
    weigh as much as the 16 SH values in the MLP's input)."""
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import lego_bitfield
    torch.manual_seed(0)
    model = NeRFNetwork(bound=bound, cuda_ray=True, density_thresh=10, bg_radius=bg_radius, **kw).to(dev)
    with torch.no_grad():
        model.encoder.embeddings.normal_(0, 0.05)
        if bg_radius > 0:
            model.encoder_bg.embeddings.normal_(0, 0.3)
    bits = bits if bits is not None else lego_bitfield(cascade=model.cascade, bound=float(bound))
    model.density_bitfield.copy_(torch.from_numpy(bits).to(dev))
    return model


def _trainer(dev, data, seed=3, options=None, model=None, M=M_ROWS, **kw):
    from nerf.fused import FusedTrainer
    return FusedTrainer(model if model is not None else _model(dev), data, M=M, seed=seed, options=options, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def _forward(model, rays_o, rays_d, table_dtype=torch.float32, rgba=None, image=None, ws=None, keep=False):
    """ngp_background_forward on the model's parameters -> bg (and x_save, sph_save with keep)."""
    import _ngp_native as nat
    eb, bn, N, dev = model.encoder_bg, model.bg_net, rays_o.shape[0], rays_o.device
    table = eb.embeddings.detach().to(table_dtype).contiguous()
    w = bn.weights.detach().half().contiguous()
    bg = torch.full((N, 3), -1.0, device=dev)
    xs = torch.zeros(N, 32, dtype=torch.float16, device=dev) if keep else None
    sp = torch.zeros(N, 2, device=dev) if keep else None
    P = nat.ptr
    nat.check(nat.lib().ngp_background_forward(
        P(rays_o), P(rays_d), float(model.bg_radius), N, P(table), nat.DTYPE_CODE[table_dtype], P(eb.offsets),
        eb.num_levels, eb.level_dim, float(np.log2(eb.per_level_scale)), eb.base_resolution, P(w), bn.input_dim,
        bn.hidden_dim, bn.num_layers, P(bg), P(rgba), P(xs), P(sp), P(image), P(ws), nat.stream_of(bg)),
        "background_forward")
    torch.cuda.synchronize()
    return (bg, xs, sp) if keep else bg


# ---- 1. forward ---------------------------------------------------------------------
def test_forward_matches_float64_and_autograd(cuda):
    """257 rays (a ragged tail past every 64-ray block and 16-ray MFMA tile),
    origins uniform in a ball of radius 2.4 inside the sphere of radius 3, unit
    directions; the background table ~ N(0, 0.3) (_model), the MLP at 4 x FFMLP's
    init (U(+-0.87): at the init itself the logits' spread is ~0.1 and the
    colours stay within 0.03 of 0.5). Bound of the float64 comparison: twice the error of the autograd ops
    (model.background under autocast) against the same float64 values, measured
    here; the kernel rounds through fp16 at different points of the same
    computation. Against the autograd ops themselves: 2 fp16 ulps of [0.5, 1)
    (2 * 2^-11): one for a logit that rounded the other way, one for the half
    sigmoid."""
    import raymarching
    N, R = 257, 3.0
    model = _model(cuda, bg_radius=R)
    with torch.no_grad():
        model.bg_net.weights.mul_(4.0)
    g = torch.Generator().manual_seed(7)
    o = torch.randn(N, 3, generator=g)
    o = (o / o.norm(dim=1, keepdim=True) * 2.4 * torch.rand(N, 1, generator=g) ** (1 / 3)).to(cuda).contiguous()
    d = torch.randn(N, 3, generator=g)
    d = (d / d.norm(dim=1, keepdim=True)).to(cuda).contiguous()
    assert float(o.norm(dim=1).max()) < R

    bg = _forward(model, o, d)
    assert torch.isfinite(bg).all() and float(bg.std()) > 0.1  # not a constant 0.5
    # the fp16 copy of the table gives the same bits as the fp32 table rounded on load
    assert torch.equal(_bits(bg), _bits(_forward(model, o, d, table_dtype=torch.float16)))

    want = bh.background64(o.cpu().numpy(), d.cpu().numpy(), R,
                           model.encoder_bg.embeddings.detach().half().cpu().numpy(),
                           model.bg_net.weights.detach().half().cpu().numpy())
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        auto = model.background(raymarching.sph_from_ray(o, d, R), d)
    model.train()
    assert auto.dtype == torch.float16 and auto.shape == (N, 3)
    err_auto = float(np.abs(auto.double().cpu().numpy() - want).max())
    err = float(np.abs(bg.double().cpu().numpy() - want).max())
    vs_auto = float((bg - auto.float()).abs().max())
    print(f"background forward, max |err| against float64: kernel {err:.3e}, autograd ops {err_auto:.3e}; "
          f"kernel against autograd ops {vs_auto:.3e}")
    assert 0 < err_auto < 2e-3
    assert err <= 2 * err_auto
    assert vs_auto <= 2 * 2.0 ** -11

    # training mode: the white-blended target, alpha 1, bit for bit; the same bg
    rgba = torch.rand(N, 4, generator=g).to(cuda)
    rgba[::5, 3] = 0.0
    rgba[1::5, 3] = 1.0
    blend = rgba[:, :3] * rgba[:, 3:] + 1 * (1 - rgba[:, 3:])
    target = rgba.clone()
    bg_t, xs, sp = _forward(model, o, d, rgba=target, keep=True)
    assert torch.equal(_bits(bg_t), _bits(bg))
    assert torch.equal(target[:, 3], torch.ones(N, device=cuda))
    assert torch.equal(_bits(target[:, :3]), _bits(blend))
    assert torch.equal(sp, (raymarching.sph_from_ray(o, d, R) + 1) / 2)
    assert float(xs[:, 24:].abs().max()) == 0 and float(xs[:, 16:24].abs().max()) > 0
    # inference blend: image += (1 - ws) * bg, on the kernel's own bg
    image, ws = torch.rand(N, 3, generator=g).to(cuda), torch.rand(N, generator=g).to(cuda)
    blended = image.clone()
    bg_i = _forward(model, o, d, image=blended, ws=ws)
    assert torch.equal(_bits(bg_i), _bits(bg))
    assert torch.equal(_bits(blended), _bits(image + (1 - ws)[:, None] * bg_i))


# ---- 2. the step against autograd -----------------------------------------------------
@pytest.mark.parametrize("color_loss_weight", [1.0, 0.5])
def test_step_matches_autograd(cuda, scenes, color_loss_weight):
    """FusedTrainer._forward_backward against Trainer._forward_backward on the
    same rays of a 32 x 32 RGBA scene, a fresh model with bg_radius 4, with
    test_depth_step_matches_autograd's bounds: loss 1e-3 relative, every
    gradient's relative L2 error below 1e-2. Trainer blends the RGBA target on
    white for a model with a background, as the fused forward does."""
    from nerf.train import Trainer
    data = _dataset(scenes["rgba32"], cuda)
    f32 = _dataset(scenes["rgba32"], cuda, store="float32")
    assert data.images.shape == (6, 32, 32, 4)
    base = _model(cuda)
    ref = copy.deepcopy(base)
    ref.mean_count = 30000
    ft = _trainer(cuda, data, model=base, color_loss_weight=color_loss_weight)
    assert len(ft.params) == 5 and ft._depth == (color_loss_weight != 1)
    ft._sample()
    ft.noises.zero_()  # the autograd step marches with perturb=False
    ft._forward_backward()
    torch.cuda.synchronize()
    gt = f32.images[int(ft.image_index)].view(-1, 4)[ft.pix.long()]
    tr = Trainer(ref, data, perturb=False, update_density=False, color_loss_weight=color_loss_weight)
    assert float(tr.scaler.get_scale()) == ft.scale
    batch = {"rays_o": ft.rays_o.clone()[None], "rays_d": ft.rays_d.clone()[None], "images": gt[None]}
    ref.train()
    loss = tr._forward_backward(batch)
    torch.cuda.synchronize()
    assert int(ft.counter[0]) == int(ref.step_counter[0, 0]) > 0
    see_through = float((1 - ft.out_ws).mean())
    assert see_through > 0.5  # most rays see the background: the comparison is not vacuous
    fused_loss, lv = float(ft.loss_ray.double().sum()) / ft.N, float(loss.detach())
    print(f"samples {int(ft.counter[0])}, mean 1 - weights_sum {see_through:.3f}, loss fused {fused_loss:.8f} "
          f"autograd {lv:.8f}")
    assert abs(fused_loss - lv) <= 1e-3 * abs(lv) + 1e-7
    refs = [ref.encoder.embeddings.grad, ref.sigma_net.weights.grad, ref.color_net.weights.grad,
            ref.encoder_bg.embeddings.grad, ref.bg_net.weights.grad]
    names = ["embeddings", "sigma_net", "color_net", "encoder_bg", "bg_net"]
    assert len(ft.grads) == 5
    for name, g, r in zip(names, ft.grads, refs):
        print(f"grad {name} rel {_rel(g, r):.3e}")
        assert torch.isfinite(g.float()).all(), name
        assert r.abs().max() > 0, name
        assert _rel(g, r) < 1e-2, (name, _rel(g, r))
    assert int(ft.state.view(torch.int32)[5]) == 0  # found_inf stays clear


# ---- 3. off means unchanged ------------------------------------------------------------
def test_off_means_unchanged(cuda, scenes):
    """bg_radius = -1: three parameter tensors, and two identical runs (8 eager
    steps, capture, 10 replayed, flush) end bit-identical. (Equality with the
    parent commit is pinned by the existing bit-exact tests.)"""
    data = _dataset(scenes["rgba32"], cuda)
    runs = []
    for _ in range(2):
        ft = _trainer(cuda, data, model=_model(cuda, bg_radius=-1))
        assert len(ft.params) == 3 and not ft._bg and not hasattr(ft, "out_ws")
        for _ in range(8):
            ft.step()
        ft.capture()
        ft.run(10)
        ft.flush()
        torch.cuda.synchronize()
        runs.append(ft)
    a, b = runs
    assert a.optimizer_steps == b.optimizer_steps > 0
    assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))
    assert not any("bg" in k for k in a.model.state_dict())


# ---- 4. graph equals eager --------------------------------------------------------------
def test_graph_equals_eager(cuda, scenes):
    """With the model on, from the same state: 3 eager steps, then 1 + 2 * 3
    more, eager in one run and (one eager step after the capture's flush-free
    warm-up, then a 3-step graph twice) in the other. The last step's forward
    outputs bg and rgba and the parameters after a flush are identical: the
    accumulation is order-independent (integer atomics), so bitwise. A forward
    ordered after the bin launch's draw, or a backward after it, would read the
    next batch's rgba / bg and differ."""
    data = _dataset(scenes["rgba32"], cuda)
    base = _model(cuda)
    out = []
    for graph in (False, True):
        ft = _trainer(cuda, data, model=copy.deepcopy(base))
        for _ in range(3):
            ft.step()
        if graph:
            ft.capture(warmup=0, multi=3)
            assert ft.graph_multi is not None
            ft.run(7)
            assert ft.eager_steps == 3
        else:
            for _ in range(7):
                ft.step()
            assert ft.eager_steps == 10
        torch.cuda.synchronize()
        fwd = (ft.bg_x.clone(), ft.out_image.clone())
        ft.flush()
        torch.cuda.synchronize()
        out.append((ft, fwd))
    (a, fa), (b, fb) = out
    assert a.optimizer_steps == b.optimizer_steps > 0
    # (the bin launch has drawn the next batch over rgba and bg: the step's own
    # forward is compared through what it kept, x_save, and the composite's image)
    assert torch.equal(_bits(fa[0].float()), _bits(fb[0].float())) and torch.equal(_bits(fa[1]), _bits(fb[1]))
    assert torch.equal(_bits(a.rgba), _bits(b.rgba)) and torch.equal(_bits(a.bg), _bits(b.bg))
    assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))
    assert float(a.params[3].detach().abs().max()) > 0
    assert not torch.equal(a.params[4].detach(), base.bg_net.weights.detach())  # the background trained


# ---- 5. found-inf -------------------------------------------------------------------------
def test_found_inf_is_raised(cuda, scenes):
    """The backward entry alone on a step's ordinary inputs with the state's
    scale at 2^40: the colour gradient overflows fp16, the flag is raised, the
    values left in the gradient regions are finite or covered by the flag, and
    the optimizer skips: no NaN parameter, the scale halves, no Adam step."""
    data = _dataset(scenes["rgba32"], cuda)
    ft = _trainer(cuda, data)
    ft._sample()
    ft._forward_backward()
    torch.cuda.synchronize()
    si, sf = ft.state.view(torch.int32), ft.state.view(torch.float32)
    assert int(si[5]) == 0 and torch.isfinite(ft.flat_grad.float()).all()
    before = ft.flat_param.clone()
    sf[0] = 2.0 ** 40
    ft._background_backward()
    torch.cuda.synchronize()
    assert int(si[5]) & 1
    assert not bool(ft.bg_scratch.any())  # the scratch is left zero
    ft._pending = True
    steps = int(si[6])
    ft._optimizer(prechecked=True)
    torch.cuda.synchronize()
    assert torch.isfinite(ft.flat_param).all() and torch.equal(_bits(ft.flat_param), _bits(before))
    assert float(sf[0]) == 2.0 ** 39 and int(si[6]) == steps and int(si[5]) == 0


# ---- 6. it learns -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def learned(cuda, scenes):
    """8 RGB views at 64 x 64 of the boxes over a smooth backdrop, one view
    held out; the occupancy fixed to a ball around the solid (no density
    updates), so the field cannot paint the backdrop; 4 eager steps + run(200),
    with bg_radius 4 and without."""
    from nerf.eval import psnr
    from nerf.provider import sphere_bitfield
    data = _dataset(scenes["sky64"], cuda)
    val = _dataset(scenes["sky64"], cuda, type="val")
    assert data.images.shape == (8, 64, 64, 3) and val.images.shape == (1, 64, 64, 3)
    out = {}
    for radius in (4, -1):
        torch.manual_seed(0)
        from nerf.network_ff import NeRFNetwork
        model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10, bg_radius=radius).to(cuda)
        model.density_bitfield.copy_(torch.from_numpy(sphere_bitfield(0.7)).to(cuda))
        ft = _trainer(cuda, data, model=model, M=4 * M_ROWS)
        for _ in range(4):
            ft.step()
        ft.capture()
        ft.run(200)
        ft.flush()
        torch.cuda.synchronize()
        errors, loss = ft.device_errors(), ft.last_loss
        model.eval()
        out[radius] = dict(model=model, psnr=psnr(model, val, 0), errors=errors, loss=loss, data=data, val=val)
        print(f"bg_radius {radius}: held-out PSNR {out[radius]['psnr']:.4f}, loss {loss:.6f}")
    return out


def test_it_learns_the_backdrop(learned):
    for r in (4, -1):
        assert learned[r]["errors"] == 0 and np.isfinite(learned[r]["loss"]) and np.isfinite(learned[r]["psnr"])
    assert learned[4]["psnr"] > learned[-1]["psnr"]


# ---- 7. frames and the command line ---------------------------------------------------------
def test_frames_blend_the_model_background(cuda, learned):
    from nerf.frames import FrameRenderer, quantise
    model, val = learned[4]["model"], learned[4]["val"]
    fr = FrameRenderer(model, val.H, val.W, val.intrinsics, bg_color=1.0)
    fr.load_weights()
    fr.capture()
    fr.set_poses(val.poses)
    rgb8, _ = fr.render(0, floats=True)
    torch.cuda.synchronize()
    r = fr.renderer
    ws = r.weights_sum
    assert float(ws.max()) > 0.5 and float(ws.min()) < 0.5
    assert float(r.bg.std()) > 0.01  # the learned backdrop, not a constant
    want = fr.loop_image + (1 - ws)[:, None] * r.bg
    assert torch.equal(_bits(fr.image), _bits(want)) and torch.equal(_bits(r.image), _bits(want))
    assert np.array_equal(rgb8.cpu().numpy(), quantise(fr.image.cpu().numpy()).reshape(val.H, val.W, 3))
    # ... and FusedRenderer.render uses the same colours as its bg_color
    out = r.render(r.rays_o.clone(), r.rays_d.clone(), bg_color=1)
    assert torch.equal(_bits(out["image"]), _bits(want))


def test_main_nerf_with_a_background(cuda, scenes, tmp_path, capsys):
    import main_nerf
    from PIL import Image
    ws = str(tmp_path / "ws")
    args = [scenes["rgba32"], "-O", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--num_rays", "256",
            "--sample_budget", "65536", "--bg_radius", "4", "--workspace", ws]
    trained = main_nerf.main([*args, "--iters", "32", "--write_frames"])
    text = capsys.readouterr().out
    assert "background model at radius 4" in text and str(697776 * 2 + 3072) in text
    assert np.isfinite(trained["psnr"]) and np.isfinite(trained["loss"])
    state = torch.load(trained["checkpoint"], map_location="cpu", weights_only=False)
    assert sorted(state["optimizer"]["state"]) == [0, 1, 2, 3, 4]
    assert [g["params"] for g in state["optimizer"]["param_groups"]] == [[0], [1], [], [2], [3], [4]]
    assert "encoder_bg.embeddings" in state["model"] and "bg_net.weights" in state["model"]
    first = [open(p, "rb").read() for p in trained["frame_paths"]]
    assert first and len(np.unique(np.asarray(Image.open(trained["frame_paths"][0])))) > 4
    out = main_nerf.main([*args, "--test"])
    assert out["frame_paths"] == trained["frame_paths"]
    assert [open(p, "rb").read() for p in out["frame_paths"]] == first


# ---- 8. checkpoint round trip -----------------------------------------------------------------
def test_checkpoint_round_trip(cuda, scenes):
    data = _dataset(scenes["rgba32"], cuda)
    a = _trainer(cuda, data)
    for _ in range(5):
        a.step()
    state = a.checkpoint()
    assert sorted(state["optimizer"]["state"]) == [0, 1, 2, 3, 4]
    assert len(state["lr_scheduler"]["base_lrs"]) == 6
    b = _trainer(cuda, data, model=_model(cuda))
    b.load_checkpoint(state)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))
    lo = a._starts[1]  # (world 1 keeps no fp16 copy of the main table)
    assert torch.equal(_bits(a.flat_half[lo:].float()), _bits(b.flat_half[lo:].float()))
    assert torch.equal(_bits(a.exp_avg), _bits(b.exp_avg)) and torch.equal(_bits(a.exp_avg_sq), _bits(b.exp_avg_sq))
    assert float(a.exp_avg[a._starts[3]:].abs().max()) > 0  # the background's moments moved
    assert a.scale == b.scale and a.optimizer_steps == b.optimizer_steps > 0
    assert int(a.state.view(torch.int32)[4]) == int(b.state.view(torch.int32)[4])  # growth tracker
    # torch's Adam over the model's own groups loads the optimizer dict
    opt = torch.optim.Adam(b.model.get_params(1e-2), lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    opt.load_state_dict(state["optimizer"])
    assert len(opt.param_groups) == 6
    got = opt.state[b.model.bg_net.weights]["exp_avg"]
    assert torch.equal(got.to(cuda).reshape(-1), a.exp_avg[a._starts[4]:a._starts[4] + 3072])
    # the optimizer part does not move between models with and without a background
    plain = _trainer(cuda, data, model=_model(cuda, bg_radius=-1))
    with pytest.raises(ValueError, match="background"):
        plain.load_checkpoint(state)
    plain.load_checkpoint(state, model_only=True)  # the model part keeps strict=False
    with pytest.raises(ValueError, match="background"):
        b.load_checkpoint(plain.checkpoint())


# ---- construction errors ----------------------------------------------------------------------
def test_construction_errors(cuda, scenes):
    data = _dataset(scenes["rgba32"], cuda)
    far = float(data.poses[:, :3, 3].norm(dim=1).max())
    assert 3 < far < 4
    with pytest.raises(ValueError, match="bg_radius 3"):
        _trainer(cuda, data, model=_model(cuda, bg_radius=3))
    with pytest.raises(ValueError, match="single-process"):
        _trainer(cuda, data, distributed=True)
    ft = _trainer(cuda, data, options=dict(march_adam=False, split_head=True))  # that path carries the launches
    ft.step()
    ft.step()
    ft.flush()
    assert ft.optimizer_steps == 2 and np.isfinite(ft.last_loss)
