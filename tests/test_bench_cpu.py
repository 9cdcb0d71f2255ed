"""bench.py command-line contract on the CPU sample config: the result line,
--steps really setting the timed step count, --full, and --dump-outputs
writing comparable float32 arrays."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
BASE = ["--gpus", "1", "--batch-size", "2", "--seq-len", "64",
        "--config", str(REPO / "configs" / "model-config-sample.yaml")]


def _run_bench(*extra):
    # CPU path on every machine: bit-repeatable, and no GPU is opened
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), *BASE, *extra],
        cwd=str(REPO), env=env, capture_output=True, text=True, timeout=300,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    return json.loads(proc.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    root = tmp_path_factory.mktemp("bench_dump")
    results = []
    for name in ("a", "b"):
        results.append(_run_bench("--steps", "3", "--warmup", "1",
                                  "--dump-outputs", str(root / name)))
    return root, results


def test_result_line_fields(dumped):
    _, (res, _) = dumped
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    # value is tokens/sec over the timed steps: batch * seq tokens per step
    toks = 2 * 64
    assert res["value"] == pytest.approx(toks / (res["ms_per_step"] / 1000.0), rel=1e-6)


def test_dump_outputs_files(dumped):
    root, (res, _) = dumped
    files = {p.stem: np.load(p) for p in (root / "a").glob("*.npy")}
    assert {"loss", "ntokens", "losses", "param_sample", "grad_sample"} <= set(files)
    total = 0
    for arr in files.values():
        assert arr.dtype in (np.float32, np.float64)
        assert np.isfinite(arr).all()
        total += arr.nbytes
    assert total <= 64 * 2**20
    assert files["losses"].shape == (3,)  # one entry per timed step
    assert files["loss"][0] == files["losses"][-1]
    assert files["loss"][0] == pytest.approx(res["config"]["final_loss"], rel=1e-6)
    assert files["param_sample"].shape == files["grad_sample"].shape
    assert np.abs(files["grad_sample"]).max() > 0


def test_dump_outputs_repeatable(dumped):
    root, _ = dumped
    for p in (root / "a").glob("*.npy"):
        np.testing.assert_array_equal(np.load(p), np.load(root / "b" / p.name))


def test_full_flag_accepted():
    res = _run_bench("--steps", "1", "--warmup", "0", "--full")
    assert res["steps"] == 1 and res["ms_per_step"] > 0
