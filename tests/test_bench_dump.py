"""bench.py --dump-outputs: the writer (CPU) and the arrays of real runs (GPU): seeded inputs give the same outputs from run to run,
--steps is the number of timed steps, and the dump stays under its 64 MB budget."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_write_outputs_small_set_is_whole(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(1)
    arrays = {"game_state": rng.random((100, 41), dtype=np.float32), "flags": rng.integers(0, 255, 100).astype(np.uint8),
              "action_mask": rng.integers(-1, 2, (100, 6)).astype(np.int8), "positions": rng.random((100, 6))}
    rep = bench.write_outputs(arrays, str(tmp_path))
    got = _load(str(tmp_path))
    assert set(got) == set(arrays) and rep["envs_kept"] == 100
    for k, a in arrays.items():
        assert got[k].dtype == (np.float64 if a.dtype == np.float64 else np.float32), k
        assert np.array_equal(got[k], a.astype(got[k].dtype)) and got[k].shape == a.shape, k


def test_write_outputs_samples_the_same_rows_within_budget(tmp_path):
    bench = _bench()
    n = 4096
    frame = (np.arange(n * 84 * 84, dtype=np.int64) % 251).astype(np.uint8).reshape(n, 84, 84, 1)
    gs = np.arange(n * 41, dtype=np.float32).reshape(n, 41)
    budget = 16 << 20   # the whole set as float32 is about 116 MB
    reps = []
    for d in ("a", "b"):
        reps.append(bench.write_outputs({"game_state": gs, "player_frame": frame}, str(tmp_path / d), budget=budget))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == {"game_state", "player_frame", "env_index"}
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= budget
    rows = a["env_index"].astype(np.int64)
    assert a["env_index"].dtype == np.float64 and 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["game_state"], gs[rows]) and np.array_equal(a["player_frame"], frame[rows].astype(np.float32))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert reps[0]["envs_kept"] == len(rows) and reps[0]["bytes"] <= budget


def test_full_is_an_option_and_off_by_default():
    bench = _bench()
    plain = bench.parse_args(["--gpus", "1", "--steps", "10", "--warmup", "2"])
    assert plain.full is False and plain.steps == 10 and plain.warmup == 2
    assert bench.parse_args(["--gpus", "1", "--steps", "10", "--warmup", "2", "--full"]).full is True


def _run(args, out_dir):
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--warmup", "3", "--preroll", "40", "--no-cpu-baseline",
                        "--async-streams", "0", "--open-loop-chunk", "0", "--dump-outputs", out_dir] + args,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dump_is_reproducible_and_steps_are_timed(tmp_path):
    """Two runs with the same arguments dump the same arrays; the line reports exactly --steps timed steps and their ms_per_step."""
    args = ["--workload", "c0", "--steps", "7", "--envs-per-gpu", "1024"]
    lines = [_run(args, str(tmp_path / d)) for d in ("a", "b")]
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == {"game_state", "entity_pos", "reward", "frames", "action_mask", "flags"}
    assert a["game_state"].shape == (1024, 41) and a["game_state"].dtype == np.float32 and a["game_state"].std() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for line in lines:
        assert line["steps"] == 7 and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 1024) < 1e-6 * 1024
        assert line["dump_outputs"]["envs_kept"] == 1024


@pytest.mark.gpu
def test_bench_dump_of_full_observations_is_sampled_within_64mb(tmp_path):
    d = str(tmp_path / "obs")
    line = _run(["--workload", "doors", "--full-obs", "--obs-overlap", "", "--steps", "4", "--envs-per-gpu", "2048"], d)
    got = _load(d)
    assert {"player_frame", "global_view", "reachability_features", "switch_states", "spatial_context", "env_index"} <= set(got)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    assert 0 < len(got["env_index"]) < 2048 and line["dump_outputs"]["envs_kept"] == len(got["env_index"])
    assert got["player_frame"].shape[1:] == (84, 84, 1) and got["player_frame"].std() > 0
