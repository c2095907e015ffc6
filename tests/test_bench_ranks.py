"""bench.py --gpus N: without a torchrun environment the
script starts N rank processes itself, and every rank searches its own slice.
Here on CPU: 2 ranks over gloo with the host build of the interpreter standing
in for the device; the reported witness (all-reduce MIN over ranks) and the
time-to-first-witness index (per-slice MIN, cross-rank early stop) must equal a
single-process search of the same ranges."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = 200
WITNESS = 0x5EED0005 % (1 << 31)      # synth.build_c5's planted index
BATCH_LOG2 = 8


def _single_process_min(begin, count):
    from mythril_amd.compiler import compile_program
    from mythril_amd.hostemu import term_values
    from mythril_amd.synth import build_c5
    from tests.fakedev import FakeDevice
    syn = build_c5(term_values, n_nodes=NODES)
    dev = FakeDevice(chunk=1 << 12)
    (found,), _ = dev.search([dev.load(compile_program(syn.conjuncts))], syn.seed, begin, count, 0)
    return found


def _run_bench(extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--host-emulator", "--dist-backend", "gloo",
           "--engine", "interp", "--nodes", str(NODES), "--batch-log2", str(BATCH_LOG2), "--steps", "1",
           "--warmup", "0", "--no-cpu-baseline"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout     # one JSON line, from rank 0 only
    return json.loads(lines[0])


def test_bench_spawns_two_ranks_and_reduces_the_minimum():
    begin = WITNESS - 300                # the planted witness falls in rank 1's slice
    out = _run_bench(["--full", "--gpus", "2", "--begin", str(begin), "--ttfw-slice-log2", "8",
                      "--ttfw-max-slices", "4", "--ttfw-begin", str(WITNESS - 700)])
    assert out["n_gpus"] == 2
    assert out["config"]["rccl_world"] == 2
    assert out["config"]["dist_backend"] == "gloo"
    single = _single_process_min(begin, 2 << BATCH_LOG2)
    assert single is not None
    assert out["config"]["witness_found_in_timed_range"] == single
    # TTFW: slices of 2 x 256 from WITNESS-700; the first hit is in slice 1
    ttfw = out["config"]["time_to_first_witness"]
    assert ttfw["index"] == _single_process_min(WITNESS - 700, 4 * (2 << 8))
    assert ttfw["candidates_searched"] == 2 * (2 << 8)
    assert out["value"] > 0 and out["scaling"] == "weak"


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """Without --full: the headline fields only, --steps timed steps, and
    --dump-outputs holds what the last timed search returned (step k of a
    one-rank run searches [begin + k * batch, begin + (k + 1) * batch))."""
    import numpy as np
    batch = 1 << BATCH_LOG2
    begin = WITNESS - 100 - 2 * batch    # warm-up step 0, timed steps 1 and 2: the witness falls in step 2
    args = ["--begin", str(begin), "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")]
    out = _run_bench(args)
    assert out["steps"] == 2 and out["config"]["evals_timed"] == 2 * batch
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "evals/s" and out["higher_is_better"] is True
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - batch) < 1e-6 * batch
    for moved in ("roofline", "cpu_baseline"):
        assert moved not in out
    assert "time_to_first_witness" not in out["config"]
    single = _single_process_min(begin + 2 * batch, batch)
    assert single is not None and out["config"]["witness_found_in_timed_range"] == single
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["found.npy", "stats.npy"]
    found = np.load(tmp_path / "out" / "found.npy")
    assert found.dtype == np.float64 and found[0] == 1 and int(found[1]) + (int(found[2]) << 32) == single
    stats = np.load(tmp_path / "out" / "stats.npy")
    assert stats.dtype == np.float64 and stats[0] == batch
    # the same arguments again: the same arrays; and a last step without a witness
    _run_bench(args[:-1] + [str(tmp_path / "again")])
    assert np.array_equal(np.load(tmp_path / "again" / "found.npy"), found)
    assert np.array_equal(np.load(tmp_path / "again" / "stats.npy"), stats)
    _run_bench(["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "none")])
    assert np.load(tmp_path / "none" / "found.npy").tolist() == [0.0, 0.0, 0.0]


def test_bench_rejects_mismatched_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_rejects_devices_with_ranks():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--devices", "2"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "exclude" in r.stderr
