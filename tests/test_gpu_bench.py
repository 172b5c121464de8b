"""GPU tier: bench.py --dump-outputs.  Two runs with the same arguments time exactly --steps steps and write the same outputs of
their last step, bit for bit; the dumped segment tables are the oracle's on the dumped hidden states."""
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


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["SYLBER_BENCH_DEBUG"] = "1"                      # stderr: one completion time per timed step
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--clip-seconds", "2", "--no-cpu-baseline", "--no-api", "--no-other-configs", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    steps = [ast.literal_eval(ln.split(":", 1)[1].strip()) for ln in r.stderr.splitlines() if ln.startswith("step completion times")]
    return json.loads(r.stdout.strip().splitlines()[-1]), steps


def test_dump_outputs_same_arguments_same_outputs(tmp_path):
    runs = [_bench(tmp_path / d) for d in ("a", "b")]
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
