"""bench.py's launch contract: `--gpus N` runs N ranks from one command."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_cmd_starts_n_ranks_on_loopback():
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launch_cmd(4, ["--gpus", "4", "--steps", "7"], 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")


def test_gpus_must_match_the_launchers_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_algorithmic_bytes_of_the_step_launches():
    """SURVEY §8(d) per-unit bytes: Adam 28 B per table value (world 1, no fp16
    table copy) and 30 B per MLP weight; march 48 B/ray + 32 B/sample; grid
    forward 588 and backward 1,100 B/sample; composite 84 B/ray + 64 B/sample."""
    import types
    import torch
    sys.path.insert(0, ROOT)
    import bench
    ft = types.SimpleNamespace(params=[torch.zeros(6119864, 2), torch.zeros(7168), torch.zeros(11264)],
                               table32=True, dp=False)
    assert bench.adam_bytes(ft) == 28 * 12239728 + 30 * 18432
    b = bench.launch_bytes(ft, 80000, 4096)
    assert b["march_rays_train+adam"] == bench.adam_bytes(ft) + 48 * 4096 + 32 * 80000
    assert b["grid_encode_backward"] == 1100 * 80000 and b["grid_encode_forward"] == 588 * 80000
    assert b["composite_loss"] == 84 * 4096 + 64 * 80000 and b["ffmlp_backward"] is None
    dp = types.SimpleNamespace(params=ft.params, table32=False, dp=True, chunk=1532288)
    assert bench.adam_bytes(dp) == 30 * 1532288
    # the table groups the sweep leaves unchanged (reads only, 16 B) or does not clear (26 B)
    idle, zg = 1000000, 2000000
    assert bench.adam_bytes(ft, (idle, zg, 12239728 // 4)) == (16 * 4 * idle + 26 * 4 * zg
                                                               + 28 * (12239728 - 4 * (idle + zg)) + 30 * 18432)
    assert bench.adam_bytes(ft, (0, 0, 12239728 // 4)) == bench.adam_bytes(ft)


def test_flat_buffer_sizes_of_configs_4_and_5():
    """The data-parallel collectives move the flat fp16 gradient / forward copy:
    table + both MLPs, 8-aligned (12,239,728 table values at log2T
    19, 39,625,280 entries x 2 at log2T 22)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench._flat_total(19) == 12239728 + 7168 + 11264
    assert bench._flat_total(22) == 2 * 39625280 + 7168 + 11264


def test_fox_leg_occupancy_is_not_degenerate():
    """The Config-3 leg's Fox-shaped occupancy gives >= 20 samples per ray at
    dt_gamma 1/128 from the bench's cameras (the Lego boxes at bound 2 gave
    2.7), counted by the oracle's march_rays_train on two poses."""
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "torch-ngp_amd")]
    import oracle
    from nerf.provider import SyntheticLego, fox_bitfield
    from nerf.utils import get_rays
    bits = fox_bitfield()
    data = SyntheticLego("cpu", num_rays=2048)
    total = 0
    for k in (10, 60):
        torch.manual_seed(k)
        r = get_rays(data.poses[k:k + 1], data.intrinsics, 800, 800, 2048)
        ro, rd = (r[n][0].numpy().astype(np.float32) for n in ("rays_o", "rays_d"))
        nears, fars = oracle.near_far_from_aabb(ro, rd, np.array([-2.0] * 3 + [2.0] * 3, np.float32), 0.2)
        out = oracle.march_rays_train(ro, rd, 2.0, bits, 2, 128, nears, fars, np.zeros(2048, np.float32),
                                      M=2048 * 1024, dt_gamma=1 / 128)
        total += int(out[4][0])
    assert total / (2 * 2048) >= 20, total / 4096


def test_dump_arrays_are_float_and_the_table_sample_is_fixed(tmp_path):
    """--dump-outputs writes DIR/<name>.npy as float32 / float64, and the hash
    table goes out as the same seeded sample of its values in every run (drawn
    without touching numpy's global generator, which the batches use)."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    a, b = bench.table_sample(12239728, "cpu"), bench.table_sample(12239728, "cpu")
    assert np.array_equal(before, np.random.get_state()[1])
    assert torch.equal(a, b) and a.numel() == bench.DUMP_TABLE_SAMPLE
    assert int(a.min()) >= 0 and int(a.max()) < 12239728 and bool((a[1:] >= a[:-1]).all())
    assert bench.table_sample(7168, "cpu") is None
    tensors = [torch.arange(12239728, dtype=torch.float32), torch.ones(7168, dtype=torch.float16),
               torch.zeros(11264)]
    arrays = bench.named_arrays("param", tensors, "cpu")
    assert sorted(arrays) == ["param_color_net", "param_sigma_net", "param_table"]
    assert np.array_equal(arrays["param_table"], a.numpy().astype(np.float32))
    arrays["ray_samples"] = np.arange(5, dtype=np.int32)
    bench.write_outputs(str(tmp_path / "out"), arrays)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == sorted(arrays)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["ray_samples"], np.arange(5)) and got["param_sigma_net"].shape == (7168,)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K` times exactly K steps, prints the
    headline with ms_per_step and none of the --full measurements, and with
    --dump-outputs leaves the last step's arrays as float .npy files."""
    import numpy as np
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--settle-steps", "4", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 7 and out["n_gpus"] == 1 and out["unit"] == "rays/s" and out["dtype"] == "fp16"
    assert out["higher_is_better"] is True and "metric" in out
    assert out["ms_per_step"] > 0
    # value = rays per step / the step time (ms_per_step is rounded to 1e-4 ms)
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 / 4096 - 1) <= 1e-4 / out["ms_per_step"] + 1e-6
    assert not {"cpu_baseline", "legs", "render", "dp_path", "touched", "kernels_ms", "density_update_ms",
                "with_density_update"} & set(out)
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert sorted(got) == ["grad_color_net", "grad_sigma_net", "grad_table", "loss", "param_color_net",
                           "param_sigma_net", "param_table", "ray_loss", "ray_samples"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    # (the loss-scaled fp16 gradient may overflow in the first steps: the scaler then skips the update)
    assert all(np.isfinite(v).all() for k, v in got.items() if not k.startswith("grad_"))
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert float(got["loss"][0]) == out["loss"] and got["ray_loss"].shape == (4096,)
    assert got["ray_samples"].sum() > 0 and np.count_nonzero(got["grad_sigma_net"]) > 0
    assert np.count_nonzero(got["param_table"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["zero1", "sparse"])
def test_bench_gpus2_gloo_runs_two_ranks(exchange):
    """`bench.py --gpus 2 --backend gloo` on the one-GPU box: both ranks run the
    data-parallel step (ZeRO-1, or the replicated step with the touched-entry
    exchange) and rank 0 reports n_gpus 2 and the 2 ranks gloo joined."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--steps", "3", "--warmup", "2", "--kernel-steps", "1", "--no-cpu", "--no-graph",
                        "--settle-steps", "2", "--exchange", exchange],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["collective"] == {"backend": "gloo", "world_size": 2, "exchange": exchange}
    assert out["value"] > 0 and out["config"]["global_batch_rays"] == 2 * out["config"]["num_rays_per_gpu"]
