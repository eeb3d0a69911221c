"""GPU: the exponential moving average of the parameters (csrc/ema.hip,
FusedTrainer(ema_decay=...)) against torch_ema's update
restated on the CPU: tmp = s - p; tmp.mul_(1 - decay); s.sub_(tmp) in float32,
bit for bit; its schedule, its checkpoint entry, and that it changes nothing
else of a training run."""
import io

import numpy as np
import pytest
import torch

from ema_helpers import bits, dataset, torch_ema_decay, torch_ema_update, trainer, write_scene

pytestmark = pytest.mark.gpu

EMA_DECAY = 0.95
VIEWS = 6  # an epoch of the 32 x 32 scene
OMDS = [np.float32(1 - 2 / 11), np.float32(0.05), np.float32(0), np.float32(1)]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("lego32")), VIEWS, 32, 32)


def _ema_update(shadow, param, n, omd):
    import _ngp_native as nat
    return nat.lib().ngp_ema_update(nat.ptr(shadow), nat.ptr(param), n, float(omd),
                                    torch.cuda.current_stream().cuda_stream)


def _values(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    v[torch.rand(n, generator=g) < 0.2] = 0.0  # exact zeros mixed in
    return v


# below a vector, each tail length, and either side of a workgroup's 256 x 4 elements
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_kernel_equals_torch_bit_for_bit(cuda, n):
    import _ngp_native as nat
    for k, omd in enumerate(OMDS):
        s, p = _values(n, 10 * n + k), _values(n, 10 * n + k + 5)
        if n >= 4:
            p[1] = s[1]  # s - p == 0
        # 8 guard elements behind the n: nothing past the end is written
        ds = torch.cat([s, torch.full((8,), 7.0)]).to(cuda)
        dp = torch.cat([p, torch.full((8,), -3.0)]).to(cuda)
        assert _ema_update(ds, dp, n, omd) == 0, nat.lib().ngp_last_error()
        want = torch_ema_update(s.clone(), p, omd)
        got = ds.cpu()
        assert torch.equal(bits(got[:n]), bits(want)), (n, float(omd))
        assert torch.equal(got[n:], torch.full((8,), 7.0)) and torch.equal(dp.cpu()[:n], p)


def test_kernel_arguments(cuda):
    import _ngp_native as nat
    buf, p = torch.arange(16, dtype=torch.float32, device=cuda), torch.ones(16, device=cuda)
    keep = buf.clone()
    err_arg = -1  # NGP_ERR_ARG
    assert _ema_update(buf[1:], p, 8, 0.5) == err_arg and b"aligned" in nat.lib().ngp_last_error()
    assert _ema_update(buf, p[1:], 8, 0.5) == err_arg
    assert _ema_update(None, p, 8, 0.5) == err_arg
    assert _ema_update(buf, p, 0, 0.5) == 0  # n = 0: nothing is launched
    assert _ema_update(buf[1:], None, 0, 0.5) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


def _epoch(ft, steps=VIEWS):
    ft.run(steps)


def test_schedule_on_the_trainer(cuda, scene):
    """Three epochs with ema_update() after each: the shadow equals a CPU
    restatement fed the parameters read after each epoch, with torch_ema's
    warm-up decays 2/11, 3/12, 4/13; from num_updates = 200 on it is 0.95."""
    ft = trainer(cuda, dataset(scene, cuda), ema_decay=EMA_DECAY)
    assert ft.ema_shadow.dtype == torch.float32 and ft.ema_shadow.shape == ft.flat_param.shape
    assert ft.num_updates == 0 and torch.equal(bits(ft.ema_shadow), bits(ft.flat_param))
    assert ft.ema_shadow.data_ptr() != ft.flat_param.data_ptr()
    shadow = ft.flat_param.cpu().clone()
    decays = []
    for e in range(3):
        _epoch(ft)
        ft.ema_update()
        assert ft.num_updates == e + 1 and not ft._pending  # the pending optimizer step was applied first
        decay = torch_ema_decay(EMA_DECAY, e + 1)
        decays.append(decay)
        param = ft.flat_param.cpu()
        assert not torch.equal(param, shadow)  # the epoch moved the parameters
        torch_ema_update(shadow, param, np.float32(1.0 - decay))
        assert torch.equal(bits(ft.ema_shadow.cpu()), bits(shadow)), e
    assert decays == [2 / 11, 3 / 12, 4 / 13]
    # the views: one per parameter, its shape, the shadow's memory
    views = ft.ema_params()
    assert [v.shape for v in views] == [p.shape for p in ft.params]
    for a, v, p in zip(ft._starts, views, ft.params):
        assert v.data_ptr() == ft.ema_shadow.data_ptr() + 4 * a
        assert torch.equal(bits(v.cpu().reshape(-1)), bits(shadow[a:a + p.numel()]))
    # the alignment padding stays zero
    used = torch.zeros(ft.total, dtype=torch.bool)
    for a, p in zip(ft._starts, ft.params):
        used[a:a + p.numel()] = True
    assert float(ft.ema_shadow.cpu()[~used].abs().sum()) == 0.0
    ft.num_updates = 200
    _epoch(ft)
    ft.ema_update()
    assert ft.num_updates == 201 and torch_ema_decay(EMA_DECAY, 201) == EMA_DECAY
    torch_ema_update(shadow, ft.flat_param.cpu(), np.float32(1.0 - EMA_DECAY))
    assert torch.equal(bits(ft.ema_shadow.cpu()), bits(shadow))


def test_ema_changes_nothing_else(cuda, scene):
    """Same seed, 2 epochs + 5 steps, one trainer with EMA and an update at
    the epoch ends: masters, moments and loss are bit-equal."""
    data = dataset(scene, cuda)
    a, b = trainer(cuda, data, ema_decay=EMA_DECAY), trainer(cuda, data)
    assert b.ema_shadow is None and b.ema_decay is None
    for ft in (a, b):
        for _ in range(2):
            _epoch(ft)
            if ft is a:
                ft.ema_update()
        ft.run(5)
        ft.flush()
    torch.cuda.synchronize()
    assert a.num_updates == 2 and not torch.equal(a.ema_shadow, a.flat_param)
    for name in ("flat_param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.float32(a.last_loss).view(np.uint32) == np.float32(b.last_loss).view(np.uint32)
    with pytest.raises(RuntimeError, match="ema_decay"):
        b.ema_update()
    with pytest.raises(RuntimeError, match="ema_decay"):
        b.ema_params()


def test_checkpoint_round_trip(cuda, scene):
    data = dataset(scene, cuda)
    a = trainer(cuda, data, ema_decay=EMA_DECAY)
    _epoch(a)
    a.ema_update()
    a.run(3)
    state = a.checkpoint()
    ema = state["ema"]
    assert sorted(ema) == ["collected_params", "decay", "num_updates", "shadow_params"]
    assert ema["decay"] == EMA_DECAY and ema["num_updates"] == 1 and ema["collected_params"] is None
    params = list(a.model.parameters())  # torch_ema's order: model.parameters()
    assert isinstance(ema["shadow_params"], list) and len(ema["shadow_params"]) == len(params) == 3
    assert [t.shape for t in ema["shadow_params"]] == [p.shape for p in params]
    for t, p, mine, view in zip(ema["shadow_params"], params, a.params, a.ema_params()):
        assert p is mine and torch.equal(bits(t), bits(view)) and t.data_ptr() != view.data_ptr()
    # the model entry stays the raw weights; a checkpoint without optimizer state carries no ema
    assert torch.equal(bits(state["model"]["sigma_net.weights"]), bits(a.params[1].detach()))
    assert not torch.equal(state["model"]["sigma_net.weights"], ema["shadow_params"][1])
    assert "ema" not in a.checkpoint(full=False)
    blob = io.BytesIO()
    torch.save(state, blob)
    blob.seek(0)
    state = torch.load(blob, map_location="cpu", weights_only=False)
    b = trainer(cuda, data, ema_decay=EMA_DECAY)
    b.load_checkpoint(state)
    assert b.num_updates == 1 and torch.equal(bits(b.ema_shadow), bits(a.ema_shadow))
    c = trainer(cuda, data)  # no EMA: the entry is ignored
    c.load_checkpoint(state)
    assert c.ema_shadow is None and c.num_updates == 0
    for ft in (a, b, c):
        _epoch(ft)
        if ft is not c:
            ft.ema_update()
        ft.flush()
    torch.cuda.synchronize()
    assert a.num_updates == b.num_updates == 2
    assert torch.equal(bits(a.ema_shadow), bits(b.ema_shadow))
    assert torch.equal(bits(a.flat_param), bits(b.flat_param))
    assert torch.equal(bits(a.flat_param), bits(c.flat_param))
    # a trainer with EMA loads a checkpoint without the entry: its shadow and counter stay
    del state["ema"]
    keep, n = b.ema_shadow.clone(), b.num_updates
    b.load_checkpoint(state)
    assert b.num_updates == n and torch.equal(bits(b.ema_shadow), bits(keep))


def test_reset_starts_the_average_from_the_current_weights(cuda, scene):
    """ema_reset(): what a run does after loading weights that came without an
    EMA. The shadow is the (flushed) parameters, the warm-up starts over."""
    ft = trainer(cuda, dataset(scene, cuda), ema_decay=EMA_DECAY)
    _epoch(ft)
    ft.ema_update()
    ft.run(4)
    assert ft._pending and not torch.equal(ft.ema_shadow, ft.flat_param)
    ft.ema_reset()
    assert ft.num_updates == 0 and not ft._pending
    assert torch.equal(bits(ft.ema_shadow), bits(ft.flat_param))
    shadow = ft.flat_param.cpu().clone()
    _epoch(ft)
    ft.ema_update()
    torch_ema_update(shadow, ft.flat_param.cpu(), np.float32(1.0 - torch_ema_decay(EMA_DECAY, 1)))
    assert torch.equal(bits(ft.ema_shadow.cpu()), bits(shadow))


def test_distributed_raises(cuda, scene):
    from nerf.fused import FusedTrainer
    from ema_helpers import M_ROWS, model
    with pytest.raises(ValueError, match="ema_decay"):
        FusedTrainer(model(cuda), dataset(scene, cuda), M=M_ROWS, distributed=True, ema_decay=EMA_DECAY)
