"""bench.py --gpus N starts and verifies N ranks (the driver's BENCH command
form `python bench.py --gpus N` as well as torchrun's).

CPU: the launch decision and the child command.  GPU: 2 ranks over gloo on
the one-GPU box against 1 rank — n_gpus, the process group and the global
model's hash (the sharded round is bit-identical at every world size)."""
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_needs_launch_without_torchrun_env():
    assert bench.needs_launch(1, env={}) is False
    assert bench.needs_launch(8, env={}) is True


def test_needs_launch_inside_torchrun():
    assert bench.needs_launch(4, env={"WORLD_SIZE": "4"}) is False
    assert bench.needs_launch(1, env={"WORLD_SIZE": "1"}) is False
    with pytest.raises(SystemExit):
        bench.needs_launch(8, env={"WORLD_SIZE": "1"})


def test_launch_command_is_torchrun_child():
    cmd = bench.launch_command(["--gpus", "8", "--steps", "3"], 8, 29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert os.path.samefile(cmd[-5], os.path.join(ROOT, "bench.py"))


def _bench(gpus, extra=(), full=True):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "1", "--warmup", "1",
           "--config", "C3", "--clients", "16", *(["--full", "--no-cpu-baseline"] if full else []), *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    return json.loads(lines[0])


@functools.lru_cache(maxsize=None)
def _full_one_rank():
    """The --full line of one rank, run once for the tests that compare with it."""
    return _bench(1)


# what a plain run's line holds; everything else is a --full diagnostic
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "process_group", "full"}


def test_full_and_dump_outputs_options():
    """--full is off by default; --dump-outputs takes a directory."""
    ap = bench.arg_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert plain.full is False and plain.dump_outputs is None and (plain.steps, plain.warmup) == (7, 3)
    args = ap.parse_args(["--full", "--dump-outputs", "some/dir"])
    assert args.full is True and args.dump_outputs == "some/dir"


def test_dump_outputs_arrays(tmp_path):
    """dump_outputs writes the round's results as float32 / float64 .npy; a
    model above DUMP_MODEL_MAX coordinates is a fixed seeded sample of it."""
    import types

    import numpy as np
    import torch
    K, P = 6, 1000
    defense = types.SimpleNamespace(distances=torch.rand(K, K, dtype=torch.float64), scores_device=torch.rand(K),
                                    order_device=torch.randperm(K))
    eng = types.SimpleNamespace(global_flat=torch.randn(P), losses=torch.rand(K), defense=defense)
    bench.dump_outputs(eng, True, str(tmp_path / "a"))
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    assert set(got) == {"global_model", "client_losses", "krum_distances", "krum_scores", "krum_order"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["global_model"], eng.global_flat.numpy())
    assert np.array_equal(got["client_losses"], eng.losses.numpy())
    assert np.array_equal(got["krum_distances"], defense.distances.numpy())
    assert np.array_equal(got["krum_order"], defense.order_device.numpy().astype(np.float64))
    bench.dump_outputs(eng, False, str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "b")) == ["client_losses.npy", "global_model.npy"]
    old, bench.DUMP_MODEL_MAX = bench.DUMP_MODEL_MAX, 100
    try:
        bench.dump_outputs(eng, False, str(tmp_path / "c"))
        bench.dump_outputs(eng, False, str(tmp_path / "d"))
    finally:
        bench.DUMP_MODEL_MAX = old
    c, d = np.load(tmp_path / "c" / "global_model.npy"), np.load(tmp_path / "d" / "global_model.npy")
    idx = np.sort(np.random.default_rng(0).choice(P, 100, replace=False))
    assert c.shape == (100,) and np.array_equal(c, d) and np.array_equal(c, eng.global_flat.numpy()[idx])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_plain_run_dumps_the_timed_rounds_model(cuda, tmp_path):
    """A plain run prints the headline fields alone and --dump-outputs writes
    the global model of its last timed round: the model whose sha256 the
    --full run of the same arguments prints."""
    import hashlib

    import numpy as np
    plain = _bench(1, ["--dump-outputs", str(tmp_path)], full=False)
    assert set(plain) == PLAIN_KEYS and plain["full"] is False
    assert plain["steps"] == 1 and plain["ms_per_step"] == pytest.approx(1e3 / plain["value"])
    full = _full_one_rank()
    assert PLAIN_KEYS < set(full) and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "config", "n_gpus"):
        assert plain[k] == full[k]
    glob = np.load(tmp_path / "global_model.npy")
    assert glob.dtype == np.float32 and glob.shape == (full["config"]["params"],)
    assert hashlib.sha256(glob.tobytes()).hexdigest() == full["global_sha256"]
    assert np.load(tmp_path / "client_losses.npy").shape == (16,)
    D = np.load(tmp_path / "krum_distances.npy")
    assert D.dtype == np.float64 and D.shape == (16, 16) and np.isfinite(D).all()
    order = np.load(tmp_path / "krum_order.npy")
    assert sorted(order.tolist()) == list(range(16))
    assert sum(tmp_path.joinpath(n).stat().st_size for n in os.listdir(tmp_path)) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_two_gloo_ranks_equal_one(cuda):
    one = _full_one_rank()
    two = _bench(2, ["--backend", "gloo"])
    print("\n[bench --gpus 1]", {k: one[k] for k in ("value", "n_gpus", "global_sha256")})
    print("[bench --gpus 2 gloo]", {k: two[k] for k in ("value", "n_gpus", "process_group", "global_sha256")})
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["process_group"] == {"backend": "gloo", "world_size": 2}
    assert two["global_sha256"] == one["global_sha256"]
    assert two["attackers_selected"] == one["attackers_selected"] == []


def test_cpu_baseline_every_aggregator():
    """cpu_baseline reports a local-update time and the
    aggregate-ms of every hot-path aggregator, for any defense (TINY model,
    small budget)."""
    from flr.models.multimodal import TINY, num_params
    P = num_params(TINY)
    out = bench.cpu_baseline(TINY, P, 8, "trimmed_mean", 1, 4, 2, 4, budget_s=2.0)
    assert set(out["aggregate_ms"]) == {"fedavg", "krum", "trimmed_mean", "median", "krum_trimmed_mean"}
    assert all(v > 0 for v in out["aggregate_ms"].values())
    assert out["aggregate_ms_this_defense"] == out["aggregate_ms"]["trimmed_mean"]
    assert out["value"] == pytest.approx(1.0 / (8 * out["local_update_s_per_client"]
                                                + out["aggregate_ms"]["trimmed_mean"] * 1e-3))
    assert out["kind"] == "port" and out["cores"] >= 1
