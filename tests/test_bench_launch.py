"""`python bench.py --gpus N` must start its own ranks (VERDICT r1 / ADVICE): rehearsed here on CPU with
the gloo backend and the numpy stand-in engine (PANDRS_BENCH_BACKEND=gloo); the record it relays is marked
as a dry run, never as a measurement."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, env_extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=240)


def test_plain_invocation_with_two_gpus_spawns_ranks():
    p = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--rows", "20000", "--groups", "500", "--cols", "2"],
             {"PANDRS_BENCH_BACKEND": "gloo"})
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["scaling"] == "weak" and "dry_run" in rec
    assert rec["value"] > 0


def test_world_size_mismatch_is_an_error():
    p = _run(["--gpus", "2"], {"PANDRS_BENCH_BACKEND": "gloo", "RANK": "0", "WORLD_SIZE": "3"})
    assert p.returncode != 0
    assert b"WORLD_SIZE" in p.stderr


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_dump_outputs_writes_the_last_step_deterministically(tmp_path):
    """--dump-outputs DIR (rehearsed with the numpy stand-in engine at world 1): float .npy files of what the last timed
    step returned, groups in key order, the same arrays from two runs with the same arguments."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "20000", "--groups", "500", "--cols", "2",
                  "--dump-outputs", str(d)],
                 {"PANDRS_BENCH_BACKEND": "gloo", "RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
                  "MASTER_PORT": str(_free_port())})
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        rec = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.strip()][-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        dumps.append({f.name: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == {"n_groups.npy", "group_rank.npy", "group_key_hi32.npy", "group_key_lo32.npy", "group_key_null.npy", "aggregates.npy"}
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    g = int(a["n_groups.npy"][0])
    assert 0 < g <= 500 and a["aggregates.npy"].shape == (8, g)        # 2 cols x sum/mean/min/max, every group fits
    key = a["group_key_hi32.npy"][0].astype(np.uint64) << np.uint64(32) | a["group_key_lo32.npy"][0].astype(np.uint64)
    assert np.all(np.diff(key) > 0)
    s, m, lo, hi = a["aggregates.npy"][:4]
    assert np.all(lo <= m) and np.all(m <= hi) and np.all(s >= lo - 1e-9)


def test_dump_outputs_samples_large_results_under_64_mb(tmp_path):
    """A result larger than the budget is written as a fixed seeded sample of the key-ordered groups."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(7)
    g = 600_000
    keys = rng.permutation(np.arange(g, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))[None, :]
    aggs = np.vstack([keys[0].astype(np.float64) + i for i in range(16)])
    outs = []
    for run, perm in (("a", np.arange(g)), ("b", rng.permutation(g))):          # the engine's group order must not matter
        d = tmp_path / run
        bench.dump_outputs(str(d), keys[:, perm], np.zeros((1, g), np.uint8), aggs[:, perm])
        assert sum(f.stat().st_size for f in d.glob("*.npy")) <= 64_000_000
        outs.append({f.name: np.load(f) for f in d.glob("*.npy")})
    a, b = outs
    assert 0 < a["group_rank.npy"].size < g and int(a["n_groups.npy"][0]) == g
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    key = a["group_key_hi32.npy"][0].astype(np.uint64) << np.uint64(32) | a["group_key_lo32.npy"][0].astype(np.uint64)
    assert np.array_equal(key, np.sort(keys[0])[a["group_rank.npy"].astype(np.int64)])
    assert np.array_equal(a["aggregates.npy"][3], key.astype(np.float64) + 3)


FULL_ONLY = ("cpu_baseline", "cpu_baseline_parallel", "cpu_baseline_typed", "cpu_baseline_join", "north_star_sum", "c1_shape_100m",
             "c2_skew_80_20", "c2_sorted", "c3", "c4_shard", "c4_one_gpu", "c5_shard", "c5_one_gpu", "join_indices_50m_5m", "c1")


def test_full_is_an_option_and_off_by_default():
    """--full is accepted (here by the rehearsal, which has nothing to add); without it a run reports no CPU baseline or extra."""
    small = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", "20000", "--groups", "500", "--cols", "2"]
    env = {"PANDRS_BENCH_BACKEND": "gloo", "RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1"}
    for argv in (small, small + ["--full"]):
        p = _run(argv, dict(env, MASTER_PORT=str(_free_port())))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        rec = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.strip()][-1])     # gloo prints a banner of its own first
        assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and not set(FULL_ONLY) & set(rec)


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone_and_full_adds_the_rest():
    """On the device, at a small size: a plain run prints the headline and the roofline figures of its own timed steps and
    nothing that takes a run of its own; --full (here without the extra configs, whose sizes are fixed at 100 M rows and
    more) adds the CPU baselines beside the same headline fields."""
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "200000", "--groups", "5000", "--cols", "2", "--cpu-sample", "50000"]
    recs = []
    for argv in (small, small + ["--full", "--no-extras"]):
        p = _run(argv, {})
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        recs.append(json.loads(lines[0]))
    plain, full = recs
    for rec in recs:
        assert rec["metric"] == "Mrows/sec groupby-agg" and rec["unit"] == "Mrows/s" and rec["higher_is_better"] is True
        assert rec["dtype"] == "f64" and rec["steps"] == 3 and rec["warmup"] == 1 and "dry_run" not in rec
        assert rec["ms_per_step"] > 0 and abs(rec["value"] - 200000 / rec["ms_per_step"] / 1e3) <= 1e-6 * rec["value"]
        assert rec["roofline"]["device_ms"] > 0 and rec["roofline"]["phase_ms"]
    assert not set(FULL_ONLY) & set(plain) and plain["roofline"]["traffic"] is None
    assert set(full) - set(plain) == {"cpu_baseline", "cpu_baseline_parallel", "cpu_baseline_typed"}
    for name in ("cpu_baseline", "cpu_baseline_parallel", "cpu_baseline_typed"):
        assert full[name]["value"] > 0 and full[name]["unit"] == "Mrows/s"
