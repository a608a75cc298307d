"""bench.py on the device at the smallest config (C1: 100 nodes, 1000 tasks):
a plain run reports the headline fields only and, with --dump-outputs, writes
the last timed cycle's decision log; --full adds the full-scan roofline, parity
and the resident session. The dumped log is the oracle's decision log, and two
runs dump the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import run_oracle

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
from kbgpu import _abi, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cycle_roofline_8d", "scan_kernel", "full_scan_mode", "parity", "resident_session",
             "cpu_baseline")


def _bench(out, *flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out), *flags], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench(d), d


def test_plain_run_is_the_headline_only(plain):
    line, d = plain
    assert all(k in line for k in HEADLINE) and line["full"] is False
    assert not [k for k in FULL_ONLY if k in line]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "placements/s"
    assert line["value"] == pytest.approx(line["decisions_per_cycle"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert sorted(os.listdir(d)) == ["decisions.npy"]


def test_dump_is_the_oracles_decision_log(plain):
    line, d = plain
    got = np.load(d / "decisions.npy")
    ref = run_oracle(synth.config_fixture(1))["decisions"]
    assert got.dtype == np.float64 and got.shape == (len(ref), 4) and len(ref) == line["decisions_per_cycle"]
    kinds = [_abi.KIND_ALLOCATE if r["kind"] == "allocate" else _abi.KIND_PIPELINE for r in ref]
    assert got[:, 2].tolist() == kinds
    assert got[:, 3].tolist() == [r["dispatched_at"] for r in ref]
    # task and node are session indices: the oracle's (task uid, node name) pairs under one renaming
    assert len({(g[0], r["task"]) for g, r in zip(got, ref)}) == len({g[0] for g in got}) == len({r["task"] for r in ref})
    assert len({(g[1], r["node"]) for g, r in zip(got, ref)}) == len({g[1] for g in got}) == len({r["node"] for r in ref})


def test_full_run_adds_the_rest_and_dumps_the_same(plain, tmp_path):
    line = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE) and line["full"] is True
    assert not [k for k in FULL_ONLY if k not in line and k != "cpu_baseline"]
    assert line["parity"]["ok"] is True
    assert np.array_equal(np.load(tmp_path / "decisions.npy"), np.load(plain[1] / "decisions.npy"))
