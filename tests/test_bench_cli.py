"""bench.py's launcher contract on a box without GPUs (CPU tier): it never oversubscribes, never falls back to the CPU,
and its FLOP accounting matches SURVEY.md §8(d)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=600, env=env)


def test_gpus_n_refuses_when_fewer_gpus_are_visible():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs visible: the refusal path does not apply")
    r = run("--gpus", "2")
    assert r.returncode == 2
    assert "refusing to oversubscribe" in r.stderr
    assert r.stdout.strip() == ""                       # no JSON line that could be mistaken for a measurement


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present")
    r = run("--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert "no CPU fallback" in r.stderr
    assert "{" not in r.stdout


def test_flop_accounting():
    sys.path.insert(0, ROOT)
    import bench
    f = bench.gemm_flops_per_forward(32)
    assert abs(sum(f.values()) - 3.6069e12) < 1e9        # 112.7 GFLOP per 10 s clip x 32
    # one 10 s clip: 499 frames; conv1 is 2 * L1 * 512 * 512 * 3
    f1 = bench.gemm_flops_per_forward(1)
    assert f1["gemm_conv1"] == 2.0 * 15999 * 512 * 512 * 3
    assert f1["gemm_ffn1"] == 9 * 2.0 * 499 * 768 * 3072
    assert len(bench.csrc_sha16()) == 16


def test_roofline_by_peak_scores_fp8_launches_against_the_fp8_peak():
    """the MXFP8 launches answer to 5 PF, the 16-bit conv stack to 2.5 PF."""
    sys.path.insert(0, ROOT)
    import bench
    fl = bench.gemm_flops_per_forward(32)
    # every launch at exactly 1000 TFLOP/s
    kernels = {k: fl[k] / 1000e12 * 1e3 for k in fl}
    r8 = bench.roofline_by_peak(kernels, 32, bench.CLIP_SAMPLES, "fp8")
    assert r8["encoder_gemms"]["peak"] == 5000.0 and abs(r8["encoder_gemms"]["frac"] - 0.2) < 1e-3
    assert r8["conv_stack_and_projection"]["peak"] == 2500.0 and abs(r8["conv_stack_and_projection"]["frac"] - 0.4) < 1e-3
    r16 = bench.roofline_by_peak(kernels, 32, bench.CLIP_SAMPLES, "bf16")
    assert r16["encoder_gemms"]["peak"] == 2500.0 and abs(r16["encoder_gemms"]["frac"] - 0.4) < 1e-3
    rs = bench.roofline_by_peak(kernels, 32, bench.CLIP_SAMPLES, "split16")
    assert abs(rs["encoder_gemms"]["issued_frac"] - 1.2) < 1e-3        # three MFMA passes per algorithmic contraction


def test_attention_roofline_accounting():
    sys.path.insert(0, ROOT)
    import bench
    r = bench.attention_roofline({"attention": 0.333}, 32, 499, "bf16")
    assert abs(r["achieved"] - 9 * 4.0 * 32 * 12 * 499 * 499 * 64 / 0.333e-3 / 1e12) < 0.1 and r["peak"] == 2500.0
    assert bench.attention_roofline({"attention": 0.38}, 32, 499, "fp8")["peak"] == 5000.0
    assert bench.attention_roofline({}, 32, 499, "bf16") is None


def test_exchange_rehearsal_child_failure_is_reported_not_raised():
    """the one-rank RCCL self-test of `other_configs` runs as a CHILD process so that a communicator that fails or hangs cannot take the
    headline line with it: without a GPU the child dies at once, and the parent gets an `error` entry (not an exception, not a fake figure)"""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU present: the child would run the real self-test")
    sys.path.insert(0, ROOT)
    import bench
    r = bench.exchange_rehearsal(timeout_s=300)
    assert set(r) == {"error"} and "self-test child" in r["error"]


def test_steps_must_be_at_least_one():
    r = run("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr
    assert "{" not in r.stdout


def test_full_is_an_option_and_off_by_default(monkeypatch):
    """a plain command line asks for the headline figure alone; --full turns every other measurement on, and a measurement asked for
    by name without it is an error, not something silently left out"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse_args()
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 5, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--agreement-clips", "8"])
    a = bench.parse_args()
    assert a.full is True and a.agreement_clips == 8
    r = run("--agreement-clips", "8")
    assert r.returncode == 2 and "--full" in r.stderr and "{" not in r.stdout


def test_dump_outputs_fits_the_budget_with_a_fixed_sample(tmp_path):
    """--dump-outputs on the default workload's four arrays (98 MB): at most 64 MB in all, small arrays whole, the large ones a
    seeded sample of rows that depends on the shapes alone, so that two runs write the same rows"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    B, T = 32, 499
    arrays = {"hidden_states": rng.standard_normal((B, T, 768), dtype=np.float32),
              "segments": rng.integers(0, T, (B, T, 2)).astype(np.float64),
              "segment_counts": rng.integers(0, T, B).astype(np.float64),
              "segment_features": rng.standard_normal((B, T, 768), dtype=np.float32)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays)
    files = sorted((tmp_path / "a").iterdir())
    assert sum(f.stat().st_size for f in files) <= bench.DUMP_BYTES
    assert shapes["segments"] == [B, T, 2] and shapes["segment_counts"] == [B]
    assert {f.name for f in files} == {"hidden_states.npy", "hidden_states_rows.npy", "segments.npy", "segment_counts.npy",
                                       "segment_features.npy", "segment_features_rows.npy"}
    for f in files:
        assert np.load(f).dtype in (np.float32, np.float64), f.name
    for name in ("hidden_states", "segment_features"):
        got, rows = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "a" / (name + "_rows.npy"))
        assert got.dtype == np.float32 and len(got) == len(rows) > 8000 and np.all(np.diff(rows) > 0)
        assert np.array_equal(got, arrays[name].reshape(-1, 768)[rows.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "segments.npy"), arrays["segments"])
    bench.dump_outputs(str(tmp_path / "b"), {k: v + 1 for k, v in arrays.items()})
    for name in ("hidden_states_rows", "segment_features_rows"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))
    bench.dump_outputs(str(tmp_path / "c"), {"x": np.arange(10, dtype=np.int32)})
    x = np.load(tmp_path / "c" / "x.npy")
    assert x.dtype == np.float64 and np.array_equal(x, np.arange(10)) and not (tmp_path / "c" / "x_rows.npy").exists()


def test_host_outputs_mark_rows_outside_the_output():
    """table slots past an utterance's count are -1, feature rows there and frames past a ragged clip's end are 0: finite, fixed values
    (not stale buffer contents)"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    hidden, feats = torch.randn(2, 5, 768), torch.randn(2, 5, 768)
    seg = torch.arange(20, dtype=torch.int64).reshape(2, 5, 2)
    out = bench.host_outputs(hidden, seg, torch.tensor([2, 0], dtype=torch.int32), feats, valid_frames=[5, 3])
    assert out["hidden_states"].dtype == np.float32 and out["segments"].dtype == np.float64
    assert np.array_equal(out["hidden_states"][0], hidden[0].numpy()) and np.array_equal(out["hidden_states"][1, :3], hidden[1, :3].numpy())
    assert (out["hidden_states"][1, 3:] == 0).all()
    assert all(np.isfinite(a).all() for a in out.values())
    assert np.array_equal(out["segments"][0, :2], seg[0, :2].numpy()) and (out["segments"][0, 2:] == -1).all()
    assert (out["segments"][1] == -1).all() and (out["segment_features"][1] == 0).all()
    assert np.array_equal(out["segment_features"][0, :2], feats[0, :2].numpy()) and (out["segment_features"][0, 2:] == 0).all()
    assert np.array_equal(out["segment_counts"], [2.0, 0.0])
