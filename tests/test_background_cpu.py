"""CPU: the background model's host side (the reference's --bg_radius): the
model's parameters, the argument checks of ngp_background_forward / _backward
(made before any device work, so they need no GPU), the optimizer sections of
the five-tensor layout and the command line."""
import os

import pytest
import torch


def _lib():
    import _ngp_native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libngp_hip.so not built (run __graft_entry__.build())")
    return nat.lib()


def test_model_shape():
    _lib()  # (FFMLP binds the library at construction)
    from nerf.network_ff import NeRFNetwork
    plain = NeRFNetwork(bound=1, cuda_ray=True, bg_radius=-1)
    assert sorted(plain.state_dict()) == sorted([
        "aabb_train", "aabb_infer", "density_grid", "density_bitfield", "step_counter", "encoder.embeddings",
        "encoder.offsets", "sigma_net.weights", "color_net.weights"])
    assert len(plain.get_params(1e-2)) == 4 and not hasattr(plain, "bg_net")
    with pytest.raises(NotImplementedError):
        super(NeRFNetwork, plain).background(None, None)
    net = NeRFNetwork(bound=1, cuda_ray=True, bg_radius=4)
    assert net.encoder_bg.embeddings.shape == (697776, 2)
    assert net.encoder_bg.offsets.tolist() == [0, 296, 7024, 173488, 697776]
    assert net.encoder_bg.base_resolution == 16 and abs(net.encoder_bg.per_level_scale - 128 ** (1 / 3)) < 1e-9
    assert net.bg_net.weights.numel() == 64 * (32 + 16)
    groups = net.get_params(1e-2)
    assert len(groups) == 6
    assert [sum(p.numel() for p in g["params"]) for g in groups] == [
        12239728, 7168, 0, 11264, 697776 * 2, 3072]
    assert set(net.state_dict()) - set(plain.state_dict()) == {
        "encoder_bg.embeddings", "encoder_bg.offsets", "bg_net.weights"}
    # the main networks do not depend on whether a background is built
    assert torch.equal(net.sigma_net.weights, plain.sigma_net.weights)
    assert torch.equal(net.color_net.weights, plain.color_net.weights)


def test_same_rng_consumption_without_a_background():
    _lib()
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(5)
    a = NeRFNetwork(bound=1, cuda_ray=True)
    ra = torch.rand(4)
    torch.manual_seed(5)
    b = NeRFNetwork(bound=1, cuda_ray=True, bg_radius=-1)
    rb = torch.rand(4)
    assert torch.equal(ra, rb) and torch.equal(a.encoder.embeddings, b.encoder.embeddings)


FWD_OK = dict(radius=4.0, N=64, levels=4, level_dim=2, in_dim=32, hidden=64, layers=2)


def _forward(lib, null=(), **kw):
    a = dict(FWD_OK, **kw)
    p = {k: (None if k in null else 4096) for k in ("rays_o", "rays_d", "table", "offsets", "weights", "bg")}
    return lib.ngp_background_forward(p["rays_o"], p["rays_d"], a["radius"], a["N"], p["table"], 1, p["offsets"],
                                      a["levels"], a["level_dim"], 7 / 3, 16, p["weights"], a["in_dim"], a["hidden"],
                                      a["layers"], p["bg"], None, None, None, None, None, None)


def _backward(lib, null=(), **kw):
    a = dict(FWD_OK, **kw)
    names = ("out_image", "out_ws", "gt", "bg", "x_save", "sph_save", "offsets", "weights", "state", "scratch",
             "grad_table", "grad_weights", "inf_flag")
    p = {k: (None if k in null else 4096) for k in names}
    return lib.ngp_background_backward(None, a["N"], p["out_image"], p["out_ws"], p["gt"], p["bg"], p["x_save"],
                                       p["sph_save"], p["offsets"], a["levels"], a["level_dim"], 7 / 3, 16,
                                       697776 * 2, p["weights"], a["in_dim"], a["hidden"], a["layers"], p["state"],
                                       1.0, a["radius"], p["scratch"], p["grad_table"], p["grad_weights"],
                                       p["inf_flag"], None)


@pytest.mark.parametrize("entry", [_forward, _backward])
def test_argument_checks(entry):
    """NGP_ERR_ARG (-1) / NGP_ERR_UNSUPPORTED (-3) before any device work: every
    call here would fault if it launched (the pointers are not device memory)."""
    lib = _lib()
    required = (("rays_o", "rays_d", "table", "offsets", "weights", "bg") if entry is _forward else
                ("out_image", "out_ws", "gt", "bg", "x_save", "sph_save", "offsets", "weights", "state", "scratch",
                 "grad_table", "grad_weights", "inf_flag"))
    for name in required:
        assert entry(lib, null=(name,)) == -1, name
        assert b"null" in lib.ngp_last_error()
    assert entry(lib, radius=0.0) == -1 and b"radius" in lib.ngp_last_error()
    assert entry(lib, radius=-1.0) == -1
    assert entry(lib, N=0) == -1
    assert entry(lib, levels=16) == -1 and entry(lib, level_dim=4) == -1
    for kw in (dict(in_dim=16), dict(hidden=32), dict(layers=3)):
        assert entry(lib, **kw) == -3, kw
        assert b"32 -> 64 -> 3" in lib.ngp_last_error()


def test_forward_blend_buffers_go_together():
    lib = _lib()
    rc = lib.ngp_background_forward(4096, 4096, 4.0, 64, 4096, 1, 4096, 4, 2, 7 / 3, 16, 4096, 32, 64, 2, 4096, None,
                                    None, None, 4096, None, None)
    assert rc == -1 and b"image and weights_sum" in lib.ngp_last_error()
    assert lib.ngp_background_scratch_bytes(697776 * 2) == (697776 * 2 + 3072) * 8


def test_shard_plan_over_five_tensors():
    from nerf.zero1 import ShardPlan
    sizes = [12239728, 7168, 11264, 697776 * 2, 3072]
    plan = ShardPlan(sizes, 1, 0)
    assert plan.starts == [0, 12239728, 12246896, 12258160, 13653712] and plan.used == 13656784
    assert plan.chunk % 64 == 0 and plan.chunk >= plan.used
    assert plan.sections(True) == [(0, plan.starts[1], False), (plan.starts[1], plan.chunk - plan.starts[1], True)]
    assert plan.sections(False) == [(0, plan.chunk, True)]
    for k, n in enumerate(sizes):
        assert plan.owned(k) == (0, n) and plan.starts[k] % 8 == 0


def test_cli_flag():
    import main_nerf
    p = main_nerf.get_parser()
    assert p.parse_args(["scene"]).bg_radius == -1
    assert p.parse_args(["scene", "--bg_radius", "32"]).bg_radius == 32
