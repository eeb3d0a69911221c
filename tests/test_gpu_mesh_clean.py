"""GPU: what mesh export does after marching cubes (csrc/mesh_clean.hip,
nerf/mesh.py components / clean / vertex_colors, save_mesh's colors /
min_faces / keep_largest, main_nerf --mesh_color / --mesh_min_faces /
--mesh_keep_largest).

The yardsticks are the numpy restatements of mesh_clean_helpers.py (held to
scipy in test_mesh_clean_cpu.py): labels, counts and the cleaned arrays must
equal them exactly. The colours are held to 255 sigmoid in float64 over every
fp16 bit pattern, and to the autograd path of the model within one level."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_helpers as mc
import mesh_helpers as mh

pytestmark = pytest.mark.gpu

SYNTHETIC = mc.synthetic_meshes()
MC_NAMES = ["mc_noise_16", "mc_two_spheres_24"]
NAMES = list(SYNTHETIC) + MC_NAMES
RULES = [dict(min_faces=1), dict(min_faces=2), dict(min_faces=50), dict(keep_largest=True)]

_CACHE = {}


def _mesh(cuda, name):
    """-> (faces int32 [T, 3], V, vertices f32, normals f32), numpy, computed once."""
    if name not in _CACHE:
        if name in SYNTHETIC:
            f, V = SYNTHETIC[name]
            v, n = mc.fake_vertices(V, seed=len(name))
        else:
            from nerf.mesh import marching_cubes
            vol, thr = (mh.noise_volume(0, 16), 0.5) if name == "mc_noise_16" else \
                (mh.two_spheres_volume((24, 24, 24)), 10.0)
            out = marching_cubes(torch.from_numpy(vol).to(cuda), thr, aabb=(-1, -1, -1, 1, 1, 1), normals=True)
            v, f, n = (t.cpu().numpy() for t in out)
            V = len(v)
        _CACHE[name] = (f, V, v, n)
    return _CACHE[name]


def _ref(name, f, V):
    key = ("ref", name)
    if key not in _CACHE:
        _CACHE[key] = mc.components_ref(f, V)
    return _CACHE[key]


def _components(cuda, f, V):
    from nerf.mesh import components
    labels, comp_faces = components(torch.from_numpy(f).to(cuda), V)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), comp_faces.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_components_equal_the_reference(cuda, name):
    f, V, _, _ = _mesh(cuda, name)
    want_l, want_c = _ref(name, f, V)
    labels, comp_faces = _components(cuda, f, V)
    assert labels.dtype == np.int32 and comp_faces.dtype == np.int32
    assert labels.shape == (V,) and comp_faces.shape == (V,)
    assert np.array_equal(labels, want_l)
    assert np.array_equal(comp_faces, want_c)
    if name == "mc_noise_16":
        assert len(np.unique(labels)) >= 24
    if name == "mc_two_spheres_24":
        assert len(np.unique(labels)) == 2
    # atomics inside, and still the same bytes
    again_l, again_c = _components(cuda, f, V)
    assert again_l.tobytes() == labels.tobytes() and again_c.tobytes() == comp_faces.tobytes()


def _clean(cuda, f, v, n, **rule):
    from nerf.mesh import clean
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (v, f, n)]
    v2, f2, n2, info = clean(*dev, **rule)
    torch.cuda.synchronize()
    return v2.cpu().numpy(), f2.cpu().numpy(), n2.cpu().numpy(), info


@pytest.mark.parametrize("name", NAMES)
def test_clean_equals_the_reference(cuda, name):
    f, V, v, n = _mesh(cuda, name)
    for rule in RULES:
        wv, wf, wn, winfo = mc.clean_ref(v, f, n, **rule)
        gv, gf, gn, info = _clean(cuda, f, v, n, **rule)
        assert gf.dtype == np.int32 and gv.dtype == np.float32 and gn.dtype == np.float32
        assert gv.shape == wv.shape and gf.shape == wf.shape and gn.shape == wn.shape, rule
        assert np.array_equal(gf, wf), rule
        assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), rule
        assert np.array_equal(gn.view(np.uint32), wn.view(np.uint32)), rule
        assert info == winfo, rule
        if name in MC_NAMES and len(gf):
            mh.assert_closed_manifold(gf, len(gv))
        av, af, an, _ = _clean(cuda, f, v, n, **rule)
        assert av.tobytes() == gv.tobytes() and af.tobytes() == gf.tobytes() and an.tobytes() == gn.tobytes()
    if name == "mc_two_spheres_24":
        assert mh.euler(_clean(cuda, f, v, n, keep_largest=True)[1]) == 2


def test_clean_without_normals_and_both_rules(cuda):
    from nerf.mesh import clean
    f, V, v, _ = _mesh(cuda, "mc_noise_16")
    v2, f2, n2, info = clean(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), min_faces=50,
                             keep_largest=True)
    wv, wf, _, winfo = mc.clean_ref(v, f, min_faces=50, keep_largest=True)
    assert n2 is None and info == winfo
    assert np.array_equal(f2.cpu().numpy(), wf) and np.array_equal(v2.cpu().numpy(), wv)
    # the largest component is smaller than min_faces: both conditions must hold, so nothing is left
    big = int(_ref("mc_noise_16", f, V)[1].max()) + 1
    v3, f3, _, info3 = clean(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda), min_faces=big,
                             keep_largest=True)
    assert v3.shape == (0, 3) and f3.shape == (0, 3) and info3["components_kept"] == 0


def test_equal_largest_components_keep_the_smaller_label(cuda):
    f, V, v, n = _mesh(cuda, "two_tetrahedra")
    gv, gf, gn, info = _clean(cuda, f, v, n, keep_largest=True)
    assert np.array_equal(gf, mc.TETRA) and np.array_equal(gv, v[:4]) and np.array_equal(gn, n[:4])
    assert info == dict(components=2, components_kept=1, vertices_dropped=4, faces_dropped=4)


def test_a_rule_that_keeps_nothing_launches_no_emit(cuda, monkeypatch):
    import _ngp_native as nat
    from nerf.mesh import clean

    def no_emit(*a):
        raise AssertionError("ngp_mesh_clean_emit called for an empty result")
    monkeypatch.setattr(nat.lib(), "ngp_mesh_clean_emit", no_emit)
    f, V, v, n = _mesh(cuda, "strip_65_random")
    dev = [torch.from_numpy(a).to(cuda) for a in (v, f, n)]
    v2, f2, n2, info = clean(*dev, min_faces=66)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and n2.shape == (0, 3)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32
    assert info == dict(components=1, components_kept=0, vertices_dropped=V, faces_dropped=65)


def test_bad_arguments_return_their_codes(cuda):
    """Argument checks only: none of these reaches a kernel (the sentinels stay)."""
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    f = torch.zeros(4, 3, dtype=torch.int32, device=cuda)
    labels = torch.full((8,), -7, dtype=torch.int32, device=cuda)
    cf = torch.full((8,), -7, dtype=torch.int32, device=cuda)
    counts = torch.full((4,), -7, dtype=torch.int64, device=cuda)
    ws_bytes = int(lib.ngp_mesh_clean_workspace_bytes(8, 4))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    out = torch.full((8, 3), -7.0, device=cuda)
    s = nat.stream_of(f)
    ARG, UNSUPPORTED = -1, -3
    assert lib.ngp_mesh_components(None, 8, 4, P(labels), P(cf), s) == ARG
    assert "null" in lib.ngp_last_error().decode()
    assert lib.ngp_mesh_components(P(f), 8, 4, None, P(cf), s) == ARG
    assert lib.ngp_mesh_components(P(f), 8, 4, P(labels), None, s) == ARG
    assert lib.ngp_mesh_components(P(f), 2 ** 31, 4, P(labels), P(cf), s) == UNSUPPORTED
    assert lib.ngp_mesh_components(P(f), 8, 2 ** 31, P(labels), P(cf), s) == UNSUPPORTED
    assert int(lib.ngp_mesh_clean_workspace_bytes(2 ** 31, 4)) == 0
    assert lib.ngp_mesh_clean_count(P(f), 8, 4, P(labels), P(cf), 1, 0, None, ws_bytes, P(counts), s) == ARG
    assert lib.ngp_mesh_clean_count(P(f), 8, 4, P(labels), P(cf), 1, 0, P(ws), ws_bytes, None, s) == ARG
    assert lib.ngp_mesh_clean_count(P(f), 8, 4, P(labels), P(cf), 1, 0, P(ws), ws_bytes - 1, P(counts), s) == ARG
    assert "workspace" in lib.ngp_last_error().decode()
    assert lib.ngp_mesh_clean_count(P(f), 2 ** 31, 4, P(labels), P(cf), 1, 0, P(ws), ws_bytes, P(counts),
                                    s) == UNSUPPORTED
    assert lib.ngp_mesh_clean_emit(None, None, P(f), 8, 4, P(ws), ws_bytes, 8, 4, P(out), None, P(f), s) == ARG
    assert lib.ngp_mesh_clean_emit(P(out), None, P(f), 8, 4, P(ws), ws_bytes, 9, 4, P(out), None, P(f), s) == ARG
    assert lib.ngp_mesh_clean_emit(P(out), None, P(f), 8, 4, P(ws), ws_bytes, 8, 4, None, None, P(f), s) == ARG
    assert lib.ngp_mesh_clean_emit(P(out), None, P(f), 8, 4, P(ws), ws_bytes, 8, 4, P(out), P(out), P(f), s) == ARG
    assert lib.ngp_mesh_color_dirs(None, 4, P(out), s) == ARG
    assert lib.ngp_mesh_color_finish(P(out), 2, 4, 1, P(ws), s) == ARG
    assert lib.ngp_mesh_color_finish(P(out), 16, 4, 1, None, s) == ARG
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((cf == -7).all()) and bool((counts == -7).all())
    assert bool((out == -7).all())
    with pytest.raises(RuntimeError, match="int32"):
        from nerf.mesh import components
        components(f.long(), 8)


# ---- the finish kernel, every fp16 bit pattern ----------------------------------

def test_finish_kernel_on_every_fp16_pattern(cuda):
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    N = 65536
    bits = np.arange(N, dtype=np.uint16)
    rows = np.full((N, 16), 0x4200, np.uint16)  # 3.0 in every other column
    shift = (0, 21845, 43690)  # every pattern passes through each of the three columns
    for m in range(3):
        rows[:, m] = np.roll(bits, -shift[m])
    logits = torch.from_numpy(rows.view(np.int16)).to(cuda).view(torch.float16)
    rgb = torch.full((N + 1, 3), 77, dtype=torch.uint8, device=cuda)
    nat.check(lib.ngp_mesh_color_finish(P(logits), 16, N, 1, P(rgb), nat.stream_of(rgb)), "mesh_color_finish")
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    assert np.all(got[N] == 77)  # nothing past the last row
    x = rows[:, :3].view(np.float16)
    s = mc.colors_ref(x)
    finite = np.isfinite(x)
    lo = np.clip(np.floor(np.where(finite, s, 0) - 1e-3), 0, 255)
    hi = np.clip(np.floor(np.where(finite, s, 0) + 1e-3), 0, 255)
    g = got[:N].astype(np.float64)
    ok = (g == lo) | (g == hi)
    assert np.all(ok[finite]), f"{(~ok & finite).sum()} finite logits off"
    print(f"finish kernel: {int((lo != hi)[finite].sum())} of {int(finite.sum())} finite values admit two bytes")
    assert np.all(got[:N][x == np.inf] == 255) and np.all(got[:N][x == -np.inf] == 0)
    assert np.all(got[:N][np.isnan(x)] == 0)
    assert finite.sum() + (x == np.inf).sum() + (x == -np.inf).sum() + np.isnan(x).sum() == 3 * N
    # logits = 0: the values are colours already, only quantised
    vals = torch.tensor([[0.0, 1.0, 0.5], [2.0, -1.0, float("nan")], [0.999, 1 / 255, 0.25]], device=cuda).half()
    out = torch.zeros(3, 3, dtype=torch.uint8, device=cuda)
    nat.check(lib.ngp_mesh_color_finish(P(vals), 3, 3, 0, P(out), nat.stream_of(out)), "mesh_color_finish")
    want = np.floor(np.clip(np.nan_to_num(vals.cpu().numpy().astype(np.float32), nan=0.0), 0, 1)
                    * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(out.cpu().numpy(), want)


def test_directions_kernel(cuda):
    import _ngp_native as nat
    lib, P = nat.lib(), nat.ptr
    n = torch.tensor([[0, 0, 2.0], [3, 4, 0], [0, 0, 0], [float("nan"), 1, 0], [float("inf"), 0, 0],
                      [-0.6, 0.0, 0.8]], device=cuda)
    d = torch.full((7, 3), 9.0, device=cuda)
    nat.check(lib.ngp_mesh_color_dirs(P(n), 6, P(d), nat.stream_of(d)), "mesh_color_dirs")
    want = np.array([[0, 0, -1], [-0.6, -0.8, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0.6, 0, -0.8], [9, 9, 9]],
                    np.float32)
    np.testing.assert_allclose(d.cpu().numpy(), want, rtol=2e-7, atol=0)


# ---- vertex_colors -------------------------------------------------------------------

def _model(cuda, seed=0, **kw):
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(seed)
    m = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10, **kw).to(cuda)
    with torch.no_grad():
        m.encoder.embeddings.normal_(0, 0.3)
    return m


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda)


def _points(cuda, V, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.rand(V, 3, generator=g) * 2 - 1).to(cuda)
    n = torch.randn(V, 3, generator=g)
    n = n / n.norm(dim=1, keepdim=True)
    if V >= 3:
        n[V // 2] = 0.0
        n[V - 1, 1] = float("nan")
    return x, n.to(cuda).contiguous()


def _rule_dirs(n):
    length = n.norm(dim=1, keepdim=True)
    ok = torch.isfinite(length) & (length > 0)
    up = torch.tensor([0.0, 0.0, 1.0], device=n.device).expand_as(n)
    return torch.where(ok, -n / length, up).contiguous()


def _autograd_colors(m, x, n):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        c = m(x, _rule_dirs(n))[1].float()
    q = (torch.nan_to_num(c, nan=0.0).clamp(0, 1) * 255.0).to(torch.uint8)
    return q.cpu().numpy().astype(np.int32)


def _agreement(got, want, what):
    diff = np.abs(got.cpu().numpy().astype(np.int32) - want)
    print(f"vertex_colors {what}: {np.mean(diff == 0):.4%} of the bytes exact, max difference {diff.max()}")
    assert diff.max() <= 1


@pytest.mark.parametrize("V,chunk", [(1, 2 ** 20), (63, 2 ** 20), (300, 128), (2 ** 20 + 5, 2 ** 20)])
def test_vertex_colors_match_the_autograd_path(cuda, model, V, chunk):
    from nerf.mesh import _fused_color_query, vertex_colors
    assert _fused_color_query(model)
    x, n = _points(cuda, V, seed=V)
    rgb = vertex_colors(model, x, n, chunk=chunk)
    assert rgb.shape == (V, 3) and rgb.dtype == torch.uint8
    want = _autograd_colors(model, x, n)
    _agreement(rgb, want, f"V = {V}, chunk {chunk}")
    assert torch.equal(vertex_colors(model, x, n, chunk=chunk), rgb)
    if V == 300:
        assert torch.equal(vertex_colors(model, x, n), rgb)  # one chunk or three: the same bytes
        flipped = vertex_colors(model, x, (-n).contiguous(), chunk=chunk)
        changed = (flipped != rgb).any(dim=1).float().mean().item()
        print(f"vertex_colors: {changed:.1%} of the vertices change colour when the normals are negated")
        assert changed > 0.5
        assert vertex_colors(model, x[:0], n[:0]).shape == (0, 3)


def test_vertex_colors_fallback_for_other_models(cuda):
    from nerf.mesh import _fused_color_query, vertex_colors
    m = _model(cuda, seed=2, hidden_dim=32)
    assert not _fused_color_query(m)
    x, n = _points(cuda, 300, seed=7)
    rgb = vertex_colors(m, x, n, chunk=128)
    _agreement(rgb, _autograd_colors(m, x, n), "fallback, V = 300, chunk 128")
    assert (vertex_colors(m, x, (-n).contiguous(), chunk=128) != rgb).any()


# ---- end to end ------------------------------------------------------------------

def test_trainer_save_mesh_cleaned_and_coloured(cuda, tmp_path):
    """The 304 fused steps of test_gpu_mesh.py's end-to-end recipe, then the
    plain export and the cleaned, coloured one at 64^3."""
    from nerf.fused import FusedTrainer
    from nerf.mesh import read_ply, sample_density, vertex_colors
    from nerf.network_ff import NeRFNetwork
    from nerf.provider import SyntheticLego
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(cuda)
    model.train()
    data = SyntheticLego(cuda, num_rays=1024)
    model.mark_untrained_grid(data.poses, data.intrinsics)
    ft = FusedTrainer(model, data, M=131072, seed=0)
    for it in range(304):
        if it % 16 == 0:
            ft.update_density()
        ft.step()
    ft.flush()
    vol = sample_density(model, 64)
    thr = 10.0
    if not bool((vol >= 10).any()):  # no sigma >= 10 yet: the median of the positive values
        thr = float(vol[vol > 0].median())
    raw, nv0, nt0 = ft.save_mesh(str(tmp_path / "raw.ply"), resolution=64, threshold=thr)
    v0, f0, n0, c0 = read_ply(raw, with_colors=True)
    assert c0 is None and v0.shape == (nv0, 3) and f0.shape == (nt0, 3)
    info = {}
    path, nv, nt = ft.save_mesh(str(tmp_path / "clean.ply"), resolution=64, threshold=thr, colors=True, min_faces=20,
                                info=info)
    v, f, n, c = read_ply(path, with_colors=True)
    print(f"end to end: threshold {thr:g}, {nv0} / {nt0} -> {nv} / {nt} vertices / triangles, {info}")
    assert v.shape == (nv, 3) and f.shape == (nt, 3) and n.shape == (nv, 3)
    assert c.shape == (nv, 3) and c.dtype == np.uint8
    wv, wf, wn, winfo = mc.clean_ref(v0, f0, n0, min_faces=20)
    assert np.array_equal(f, wf) and info == winfo
    assert np.array_equal(v.view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(n.view(np.uint32), wn.view(np.uint32))
    # the colours are those of the flushed model at the vertices that were written
    again = vertex_colors(model, torch.from_numpy(v).to(cuda), torch.from_numpy(n).to(cuda))
    assert np.array_equal(again.cpu().numpy(), c)
    if nv:
        assert len(np.unique(c.reshape(-1))) > 1
    assert len(read_ply(path)) == 3
    assert ft.device_errors() == 0


def _write_scene(path, n, H, W):
    """n RGBA training views of the Lego boxes (and the first as the val split),
    as tests/test_gpu_mesh.py writes its scene."""
    from PIL import Image

    from nerf.provider import SyntheticLego
    from nerf.utils import get_rays
    lego = SyntheticLego(torch.device("cpu"), H=H, W=W, n_poses=n, num_rays=1024)
    frames = []
    for k in range(n):
        rays = get_rays(lego.poses[k:k + 1], lego.intrinsics, H, W, -1)
        rgba = lego.target(rays["rays_o"], rays["rays_d"]).reshape(H, W, 4)
        img = (rgba.numpy() * 255).round().astype(np.uint8)
        Image.fromarray(img, "RGBA").save(os.path.join(path, f"r_{k}.png"))
        P = lego.poses[k].numpy()
        c2w = np.eye(4)
        c2w[0], c2w[1], c2w[2] = P[2], P[0], P[1]
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./r_{k}", "transform_matrix": c2w.tolist()})
    for sp, fr in (("train", frames), ("val", frames[:1])):
        with open(os.path.join(path, f"transforms_{sp}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112, "frames": fr}, f)
    return str(path)


def test_main_nerf_mesh_flags(cuda, tmp_path, capsys):
    import main_nerf
    from nerf.mesh import read_ply
    scene = tmp_path / "scene"
    scene.mkdir()
    _write_scene(str(scene), 6, 32, 32)
    common = [str(scene), "-O", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0", "--num_rays", "1024",
              "--sample_budget", "131072", "--save_mesh", "--mesh_resolution", "32", "--mesh_threshold", "0.5",
              "--iters", "32"]
    ws = str(tmp_path / "ws")
    out = main_nerf.main(common + ["--workspace", ws, "--mesh_color", "--mesh_min_faces", "4", "--mesh_keep_largest"])
    text = capsys.readouterr().out
    assert out["mesh"] == os.path.join(ws, "meshes", "ngp.ply") and os.path.exists(out["mesh"])
    assert f"{out['mesh_vertices']} vertices, {out['mesh_triangles']} triangles" in text and out["mesh"] in text
    assert out["mesh_components"] >= out["mesh_components_kept"] and out["mesh_components_kept"] in (0, 1)
    assert f"{out['mesh_components_kept']} of {out['mesh_components']} components kept" in text
    assert "vertex colours" in text
    v, f, n, c = read_ply(out["mesh"], with_colors=True)
    assert v.shape == (out["mesh_vertices"], 3) and f.shape == (out["mesh_triangles"], 3)
    assert n.shape == v.shape and c.shape == v.shape and c.dtype == np.uint8
    if len(f):
        assert f.min() == 0 and f.max() == len(v) - 1
        assert len(np.unique(mc.components_ref(f, len(v))[0])) == 1
    # the same command line without the three flags: the file and the result of before
    ws2 = str(tmp_path / "ws2")
    plain = main_nerf.main(common + ["--workspace", ws2])
    text2 = capsys.readouterr().out
    assert "mesh_components" not in plain and "components kept" not in text2 and "vertex colours" not in text2
    assert f"{plain['mesh_vertices']} vertices, {plain['mesh_triangles']} triangles" in text2
    v2, f2, n2, c2 = read_ply(plain["mesh"], with_colors=True)
    assert c2 is None and n2.shape == v2.shape == (plain["mesh_vertices"], 3)
    assert len(read_ply(plain["mesh"])) == 3
    header = open(plain["mesh"], "rb").read().split(b"end_header\n")[0]
    assert b"uchar red" not in header
