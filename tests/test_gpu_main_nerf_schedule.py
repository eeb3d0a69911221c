"""GPU: main_nerf's epoch schedule: --ema_decay,
--eval_interval with the best checkpoint, --resume and --test --ckpt best, on a
64 x 64 scene of 8 training views and 1 held-out view, 48 steps = 6 epochs."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import ema_helpers as eh

pytestmark = pytest.mark.gpu

ARGS = ["-O", "--num_rays", "1024", "--sample_budget", "131072", "--bound", "1", "--scale", "1.0", "--dt_gamma", "0"]
FLAGS = ["--ema_decay", "0.95", "--eval_interval", "2"]
NAMES = ("encoder.embeddings", "sigma_net.weights", "color_net.weights")


def _main(argv):
    """main_nerf.main(argv) -> (its result, what it printed)."""
    import main_nerf
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = main_nerf.main(argv)
    return out, text.getvalue()


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def _model(cuda, state_dict):
    """The model main_nerf builds, holding a checkpoint's weights and buffers."""
    from nerf.network_ff import NeRFNetwork
    model = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=True, density_scale=1, min_near=0.2,
                        density_thresh=10).to(cuda)
    model.load_state_dict(state_dict, strict=False)
    model.eval()
    return model


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    path = eh.write_scene(str(tmp_path_factory.mktemp("lego64")), 8, 64, 64, heldout=1)
    # the held-out view is also the test path of --test
    shutil.copy(os.path.join(path, "transforms_val.json"), os.path.join(path, "transforms_test.json"))
    return path


@pytest.fixture(scope="module")
def ema_run(cuda, scene, tmp_path_factory):
    """The run with both flags, made once: (result, printed text, workspace,
    the EMA weights each validation pass was given)."""
    from nerf.eval import Validator
    ws = str(tmp_path_factory.mktemp("ws_ema"))
    sources, run = [], Validator.run

    def spy(self, source=None, views=None):
        sources.append(None if source is None else [t.detach().cpu().clone() for t in source])
        return run(self, source=source, views=views)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Validator, "run", spy)
        out, text = _main([scene, *ARGS, "--iters", "48", "--workspace", ws, *FLAGS])
    return out, text, ws, sources


def test_ema_and_validation_every_second_epoch(cuda, scene, ema_run):
    from nerf.eval import psnr
    from nerf.fused_render import FusedRenderer
    out, text, ws, sources = ema_run
    lines = [ln for ln in text.splitlines() if "validation PSNR" in ln]
    assert len(lines) == 3 and [ln.split()[2] for ln in lines] == ["2", "4", "6"], text
    assert all(ln.rstrip().endswith("s)") for ln in lines)
    state = _load(out["checkpoint"])
    assert out["checkpoint"] == os.path.join(ws, "checkpoints", "ngp.pth")
    assert state["global_step"] == 48 and state["epoch"] == 6
    stats = state["stats"]
    assert len(stats["valid_loss"]) == 3 and all(np.isfinite(stats["valid_loss"]))
    assert len(out["valid_psnr"]) == 3 and stats["best_result"] == max(out["valid_psnr"])
    assert stats["results"] == [out["psnr"]]
    ema = state["ema"]
    assert ema["num_updates"] == 6 and ema["decay"] == 0.95 and ema["collected_params"] is None
    assert [tuple(t.shape) for t in ema["shadow_params"]] == [tuple(state["model"][k].shape) for k in NAMES]
    assert not torch.equal(ema["shadow_params"][0], state["model"][NAMES[0]])  # model: the raw weights

    # the best checkpoint: the model alone, the EMA weights of the best epoch, no density grid
    best_path = os.path.join(ws, "checkpoints", "ngp_best.pth")
    assert out["best_checkpoint"] == best_path and os.path.exists(best_path)
    best = _load(best_path)
    for key in ("optimizer", "lr_scheduler", "scaler", "ema"):
        assert key not in best
    assert "density_grid" not in best["model"] and "density_grid" in state["model"]
    assert "density_bitfield" in best["model"]
    unmapped = torch.load(best_path, weights_only=False)  # the EMA weights are stored as host tensors
    assert all(unmapped["model"][name].device.type == "cpu" for name in NAMES)
    k = int(np.argmax(out["valid_psnr"]))  # (the first of equal maxima: a later pass has to beat it)
    assert len(sources) == 3 and all(s is not None for s in sources)
    assert best["epoch"] == 2 * (k + 1) and best["stats"]["best_result"] == out["valid_psnr"][k]
    for name, shadow in zip(NAMES, sources[k]):
        assert torch.equal(eh.bits(best["model"][name]), eh.bits(shadow)), name
    # the last pass saw the shadow ngp.pth carries (no step after the sixth epoch's update)
    for a, b in zip(sources[2], ema["shadow_params"]):
        assert torch.equal(eh.bits(a), eh.bits(b))

    # the returned PSNR is the EMA weights': recomputed from the checkpoint's shadow
    model = _model(cuda, state["model"])
    val = eh.dataset(scene, cuda, type="val")
    assert val.poses.shape[0] == 1
    r = FusedRenderer(model, val.H * val.W, max_steps=1024, dt_gamma=0.0)
    r.load_weights([t.to(cuda) for t in ema["shadow_params"]])
    from_shadow = psnr(model, val, 0, dt_gamma=0.0, renderer=r)
    r.load_weights()
    from_raw = psnr(model, val, 0, dt_gamma=0.0, renderer=r)
    assert out["psnr"] == from_shadow != from_raw


def test_flags_leave_training_unaffected(cuda, scene, ema_run, tmp_path):
    """The same command without the two flags: bit-identical parameters."""
    ws = str(tmp_path / "ws")
    out, text = _main([scene, *ARGS, "--iters", "48", "--workspace", ws])
    assert "validation PSNR" not in text and out["best_checkpoint"] is None and out["valid_psnr"] == []
    assert os.listdir(os.path.join(ws, "checkpoints")) == ["ngp.pth"]
    plain, with_flags = _load(out["checkpoint"]), _load(ema_run[0]["checkpoint"])
    assert "ema" not in plain and plain["global_step"] == 48 and plain["stats"]["valid_loss"] == []
    for name in NAMES:
        assert torch.equal(eh.bits(plain["model"][name]), eh.bits(with_flags["model"][name])), name
    for i in range(3):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(eh.bits(plain["optimizer"]["state"][i][key]),
                               eh.bits(with_flags["optimizer"]["state"][i][key])), (i, key)
    assert out["psnr"] != ema_run[0]["psnr"]  # ... and is scored on the raw weights


def test_resume(cuda, scene, tmp_path):
    ws = str(tmp_path / "ws")
    missing = os.path.join(ws, "checkpoints", "ngp.pth")
    with pytest.raises(SystemExit) as e:
        _main([scene, *ARGS, "--iters", "48", "--workspace", ws, *FLAGS, "--resume"])
    assert missing in str(e.value)
    with pytest.raises(SystemExit) as e:
        _main([scene, *ARGS, "--iters", "48", "--workspace", ws, *FLAGS, "--resume", "--ckpt",
               str(tmp_path / "other.pth")])
    assert str(tmp_path / "other.pth") in str(e.value)

    first, _ = _main([scene, *ARGS, "--iters", "24", "--workspace", ws, *FLAGS])
    half = _load(first["checkpoint"])
    assert first["start_step"] == 0 and half["global_step"] == 24 and half["epoch"] == 3
    assert half["ema"]["num_updates"] == 3 and len(half["stats"]["valid_loss"]) == 1

    out, text = _main([scene, *ARGS, "--iters", "48", "--workspace", ws, *FLAGS, "--resume"])
    assert out["start_step"] == 24 and f"resumed {missing} at step 24" in text
    assert "step 48/48" in text and "trained 24 steps" in text
    state = _load(out["checkpoint"])
    assert state["global_step"] == 48 and state["epoch"] == 6 and state["ema"]["num_updates"] == 6
    # the statistics carry over: epoch 2's pass of the first run, then epochs 4 and 6
    assert [ln.split()[2] for ln in text.splitlines() if "validation PSNR" in ln] == ["4", "6"]
    assert len(state["stats"]["valid_loss"]) == 3
    assert state["stats"]["valid_loss"][0] == half["stats"]["valid_loss"][0]
    assert state["stats"]["results"] == [first["psnr"], out["psnr"]]
    assert state["stats"]["best_result"] >= half["stats"]["best_result"]
    assert not torch.equal(state["model"][NAMES[0]], half["model"][NAMES[0]])  # it trained on
    # a best checkpoint holds no optimizer state: it is not trained on
    with pytest.raises(SystemExit) as e:
        _main([scene, *ARGS, "--iters", "48", "--workspace", ws, "--resume", "--ckpt", "best"])
    assert "ngp_best.pth" in str(e.value)


def test_resume_of_a_run_that_counted_no_epochs(cuda, scene, tmp_path):
    """A plain run's checkpoint (epoch 0 at step 24, no `ema`) resumed with
    both flags: the position in the epoch follows from the step count, so the
    run ends at --iters, and the average starts from the loaded weights."""
    ws = str(tmp_path / "ws")
    first, _ = _main([scene, *ARGS, "--iters", "24", "--workspace", ws])
    half = _load(first["checkpoint"])
    assert half["global_step"] == 24 and half["epoch"] == 0 and "ema" not in half
    out, text = _main([scene, *ARGS, "--iters", "48", "--workspace", ws, *FLAGS, "--resume"])
    assert out["start_step"] == 24 and "at step 24 (epoch 3" in text and "carries no EMA" in text
    assert "step 48/48" in text and "trained 24 steps" in text
    state = _load(out["checkpoint"])
    assert state["global_step"] == 48 and state["epoch"] == 6
    assert state["optimizer"]["state"][1]["step"] <= 48
    assert [ln.split()[2] for ln in text.splitlines() if "validation PSNR" in ln] == ["4", "6"]
    assert len(state["stats"]["valid_loss"]) == 2
    assert state["ema"]["num_updates"] == 3  # epochs 4, 5 and 6


def _decode(paths):
    return [np.array(Image.open(p)) for p in paths]


def test_test_mode_renders_the_best_and_the_ema_weights(cuda, scene, ema_run):
    from nerf.frames import FrameRenderer
    _, _, ws, _ = ema_run
    test = eh.dataset(scene, cuda, type="test")
    assert test.poses.shape[0] == 1

    def frames(model, source=None):
        fr = FrameRenderer(model, test.H, test.W, test.intrinsics, dt_gamma=0.0)
        fr.load_weights(source)
        fr.set_poses(test.poses)
        return [t.cpu().numpy().copy() for t in fr.render(0)]

    out, text = _main([scene, *ARGS, "--test", "--ckpt", "best", "--workspace", ws])
    best_path = os.path.join(ws, "checkpoints", "ngp_best.pth")
    assert out["checkpoint"] == best_path and "EMA weights" not in text and out["frames"] == 1
    files = _decode(out["frame_paths"])
    want = frames(_model(cuda, _load(best_path)["model"]))
    assert files[0].shape == (64, 64, 3) and len(np.unique(files[0])) > 2
    assert np.array_equal(files[0], want[0]) and np.array_equal(files[1], want[1])

    # a full checkpoint that carries `ema`: its shadow is what is rendered
    out, text = _main([scene, *ARGS, "--test", "--workspace", ws])
    state = _load(os.path.join(ws, "checkpoints", "ngp.pth"))
    assert out["checkpoint"].endswith("ngp.pth") and "EMA weights" in text
    files = _decode(out["frame_paths"])
    model = _model(cuda, state["model"])
    want = frames(model, [t.to(cuda) for t in state["ema"]["shadow_params"]])
    raw = frames(model)
    assert np.array_equal(files[0], want[0]) and np.array_equal(files[1], want[1])
    assert not np.array_equal(want[0], raw[0])
