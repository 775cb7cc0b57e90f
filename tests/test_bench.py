"""bench.py's bookkeeping on CPU: the PMC profile is used only for the build it was measured on,
the CPU baseline's core count, the algorithmic byte counts of SURVEY.md §8(d), the output dump;
on the GPU, what a plain run and a --full run step and report."""
import json
import os

import pytest

import bench


def test_pmc_profile_only_for_the_build_it_was_measured_on(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    entry = {"hbm_bytes_per_launch": 1.0, "profile": "rX", "so_sha16": "0" * 16}
    (prof / "pmc_traffic.json").write_text(json.dumps({"config4_f64": entry}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "lib_sha16", lambda: "f" * 16)
    pmc, note = bench.read_pmc("f64", 4)
    assert pmc is None and "another build" in note
    monkeypatch.setattr(bench, "lib_sha16", lambda: "0" * 16)
    pmc, note = bench.read_pmc("f64", 4)
    assert pmc == entry and "rX" in note
    pmc, note = bench.read_pmc("f32", 4)
    assert pmc is None and "no PMC profile" in note


def test_host_threads_honours_the_granted_share(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "16")
    assert bench.host_threads() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert bench.host_threads() == (os.cpu_count() or 1)


def test_algorithmic_bytes_per_vehicle():
    # f64: 11 reals + 3 int32 + 4 uint8 read, 10 reals + 3 int32 + 2 uint8 written (one fused launch)
    assert bench.state_bytes("f64") == (11 * 8 + 12 + 4, 10 * 8 + 12 + 2)
    assert bench.state_bytes("f32") == (11 * 4 + 12 + 4, 10 * 4 + 12 + 2)


def test_configs_match_baseline_json():
    base = json.load(open(os.path.join(bench.ROOT, "BASELINE.json")))
    assert len(base["configs"]) == 5
    assert (bench.CONFIGS[4]["num_envs"], bench.CONFIGS[4]["vehicles"]) == (4096, 64)
    assert (bench.CONFIGS[2]["num_envs"], bench.CONFIGS[2]["vehicles"]) == (4096, 32)
    assert (bench.CONFIGS[3]["num_envs"], bench.CONFIGS[3]["vehicles"]) == (4096, 128)
    assert (bench.CONFIGS[5]["num_envs"], bench.CONFIGS[5]["vehicles"]) == (8192, 64)
    assert (bench.CONFIGS[1]["num_envs"], bench.CONFIGS[1]["vehicles"]) == (1, 50)
    assert bench.CONFIGS[3]["obs"]["type"] == "OccupancyGrid"


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: every tensor of the step's result as <name>.npy in float32 / float64; above
    the byte budget the large arrays keep one fixed, seeded sample of their rows, the same on every call."""
    import numpy as np
    import torch
    E = 512
    obs = torch.arange(E * 700, dtype=torch.float32).reshape(E, 7, 100)
    info = {"speed": torch.ones(E, dtype=torch.float64), "crashed": torch.zeros(E, dtype=torch.uint8),
            "action": torch.zeros(E, dtype=torch.int32), "rewards": {"collision_reward": torch.zeros(E)}}
    last = (obs, torch.ones(E), torch.zeros(E, dtype=torch.bool), torch.ones(E, dtype=torch.bool), info)
    tensors = bench.step_outputs(last, actions=torch.arange(E, dtype=torch.int32))
    assert sorted(tensors) == ["actions", "info_crashed", "info_rewards_collision_reward", "info_speed", "obs",
                               "reward", "terminated", "truncated"]
    shapes = bench.dump_outputs(str(tmp_path / "a"), tensors)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == sorted(tensors) and shapes["obs"] == [E, 7, 100]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["obs"], obs.numpy()) and got["info_speed"].dtype == np.float64
    assert np.array_equal(got["actions"], np.arange(E)) and got["truncated"].all() and not got["terminated"].any()
    # over the budget: obs (1.4 MB) is sampled by rows, the small arrays are written whole
    monkeypatch.setattr(bench, "DUMP_BUDGET", 500_000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), tensors)
    files = sorted(os.listdir(tmp_path / "b"))
    assert "sample_rows.npy" in files
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 500_000
    rows = np.load(tmp_path / "b" / "sample_rows.npy").astype(np.int64)
    assert 100 < len(rows) < E and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "obs.npy"), obs.numpy()[rows])
    assert np.load(tmp_path / "b" / "reward.npy").shape == (E,)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f)), f


def _main_line(monkeypatch, capsys, *argv):
    """bench.main() in this process (one env: config 1); its JSON line."""
    import sys
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "1", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, monkeypatch, capsys, hip_device):
    """A plain run times exactly --steps steps and reports no roofline or CPU baseline; --full adds
    them; --dump-outputs writes the last timed step's results, identical from run to run."""
    import numpy as np
    from topotrafficrl_amd.envs import VecHighwayEnv
    steps = []
    orig = VecHighwayEnv.step
    monkeypatch.setattr(VecHighwayEnv, "step", lambda self, a: (steps.append(1), orig(self, a))[1])
    out = _main_line(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "a"))
    assert len(steps) == 5 and out["steps"] == 3 and out["warmup"] == 2
    assert "roofline" not in out and "cpu_baseline" not in out
    assert out["ms_per_step"] > 0 and out["unit"] == "vehicle-steps/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64" and abs(out["value"] - 50 * 15 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    _main_line(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and {"obs.npy", "reward.npy", "terminated.npy",
                                                            "truncated.npy", "info_speed.npy"} <= set(names)
    assert sorted(out["dumped_outputs"]) == [n[:-4] for n in names]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), n
    assert np.load(tmp_path / "a" / "obs.npy").shape == (1, 5, 5)
    del steps[:]
    full = _main_line(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert len(steps) == 5 + 3 + 3  # the launch-time steps: 3 to settle + min(steps, 20) bracketed
    assert full["roofline"]["kernel_ms"] > 0 and "cpu_baseline" not in full


def _run_bench(*argv, env_extra=None):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(bench.ROOT, "bench.py"), *argv], capture_output=True,
                       text=True, env=env, timeout=240)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr


def test_gpus_n_runs_n_ranks_from_a_plain_invocation():
    """`python bench.py --gpus 2` (how the driver may call it) runs a 2-rank torch.distributed.run
    child job; the parent imports no torch (so it opens no device) and relays rank 0's line, which
    reports n_gpus == 2 with the weak-scaling shards [r*E, (r+1)*E)."""
    rc, out, err = _run_bench("--gpus", "2", "--dry-run")
    assert rc == 0, err
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    assert [tuple(s) for s in out["shards"]] == [(0, 4096), (4096, 4096)]
    assert out["launcher"]["ranks"] == 2 and out["launcher"]["parent_imported_torch"] is False
    assert out["max_elapsed"] == 0.002  # the max over both ranks


def test_strong_scaling_splits_the_global_batch():
    rc, out, err = _run_bench("--gpus", "2", "--dry-run", "--strong")
    assert rc == 0, err
    assert out["scaling"] == "strong" and out["global_envs"] == 32768
    assert [tuple(s) for s in out["shards"]] == [(0, 16384), (16384, 16384)]
    rc, out, err = _run_bench("--gpus", "1", "--dry-run", "--strong", "--global-envs", "1000")
    assert rc == 0 and out["n_gpus"] == 1 and [tuple(s) for s in out["shards"]] == [(0, 1000)]


def test_world_size_must_equal_gpus():
    rc, out, err = _run_bench("--gpus", "2", "--dry-run", env_extra={"WORLD_SIZE": "1"})
    assert rc == 2 and "WORLD_SIZE=1" in err
