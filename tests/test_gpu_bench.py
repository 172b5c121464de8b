"""GPU tier: bench.py --dump-outputs.  Two runs with the same arguments time exactly --steps steps and write the same outputs of
their last step, bit for bit; the dumped segment tables are the oracle's on the dumped hidden states.  A plain run ends with its
headline figure; --full adds the other measurements to the same line."""
import ast
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import segment_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hidden_states", "segments", "segment_counts", "segment_features")


def _bench(out_dir, extra=("--no-cpu-baseline", "--no-api", "--no-other-configs")):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["SYLBER_BENCH_DEBUG"] = "1"                      # stderr: one completion time per timed step
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--clip-seconds", "2", "--dump-outputs", str(out_dir)] + list(extra),
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    steps = [ast.literal_eval(ln.split(":", 1)[1].strip()) for ln in r.stderr.splitlines() if ln.startswith("step completion times")]
    return json.loads(r.stdout.strip().splitlines()[-1]), steps


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """two plain runs with the same arguments (shared by the tests below): (directory, [(line, steps), (line, steps)])"""
    d = tmp_path_factory.mktemp("bench")
    return d, [_bench(d / x) for x in ("a", "b")]


def test_dump_outputs_same_arguments_same_outputs(plain_runs):
    tmp_path, runs = plain_runs
    for line, steps in runs:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert [len(s) for s in steps] == [3]            # the one timed region of a one-GPU run: exactly --steps steps
        d = line["dump_outputs"]
        assert "error" not in d and d["path"] == "resident"
        assert d["arrays"]["hidden_states"] == [4, 99, 768] and d["arrays"]["segments"] == [4, 99, 2]
    got = {}
    for name in NAMES:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), name
        got[name] = a
    assert np.isfinite(got["hidden_states"]).all()
    for i, n in enumerate(got["segment_counts"].astype(np.int64)):
        exp = segment_oracle.get_segment(got["hidden_states"][i], 2.6, 0.8).reshape(-1, 2)
        assert np.array_equal(got["segments"][i, :n], exp) and (got["segments"][i, n:] == -1).all()
        assert (got["segment_features"][i, n:] == 0).all()


HEADLINE = ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data", "config")


def test_plain_run_is_lean_and_full_adds_the_rest(plain_runs):
    """a plain run carries the headline figure and none of the measurements that take passes of their own; --full (here without its
    three slowest parts) adds them to the same line, times the same steps and computes the same outputs"""
    tmp_path, runs = plain_runs
    plain = runs[0][0]
    assert plain["full"] is False and plain["value"] > 0
    for key in ("roofline", "roofline_frontend", "cpu_baseline", "api_level", "segments_per_clip"):
        assert plain[key] is None, key
    assert plain["kernel_ms_per_forward"] == {}
    for key in ("box_speed", "other_configs", "segment_agreement"):
        assert key not in plain, key
    full, steps = _bench(tmp_path / "full", ("--full", "--no-cpu-baseline", "--no-api", "--no-other-configs"))
    assert full["full"] is True and full["value"] > 0 and [len(s) for s in steps] == [3]
    for key in HEADLINE:
        assert full[key] == plain[key], key
    assert full["roofline"]["achieved"] > 0 and full["roofline_frontend"]["achieved"] > 0
    assert full["kernel_ms_per_forward"]["attention"] > 0 and full["box_speed"]["gemm_4096_cubed_tflops"] > 0
    assert full["segments_per_clip"]["max"] >= full["segments_per_clip"]["min"] >= 0
    assert full["cpu_baseline"] is None and full["api_level"] is None and "other_configs" not in full
    for name in NAMES:
        assert np.array_equal(np.load(tmp_path / "full" / (name + ".npy")), np.load(tmp_path / "a" / (name + ".npy"))), name
