"""CPU tier: sylber_amd/csrc/powf_half.h (the device restatement of glibc powf(x, .5f) that the
segmentation kernel needs for numpy's scalar `** .5`) against the host libm."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replica_matches_libm(tmp_path):
    exe = str(tmp_path / "powf_check")
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp",
                           os.path.join(ROOT, "tests", "powf_replica_check.c"), "-o", exe, "-lm"])
    stride = "1" if os.environ.get("SYLBER_EXHAUSTIVE") == "1" else "61"
    out = subprocess.run([exe, stride], capture_output=True, text=True)
    n, bad = (int(x) for x in out.stdout.split())
    assert out.returncode == 0 and bad == 0 and n > 3e7, out.stdout


def test_one_division_merge_quotient_is_the_ieee_quotient(tmp_path):
    """the merge update's one-division form (segment.hip merge_update) against a / c1 on the host: every divisor 2..8192 and every 7th of
    8193..20000 (an utterance beyond 8192 frames divides by more), 2000 x 5 dividends each (all binades of [2^-100, 2^126], the binades
    activations live in, and dividends built to put the quotient next to a rounding boundary), the ends of the range.  No mismatch allowed."""
    exe = str(tmp_path / "merge_quotient_check")
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp",
                           os.path.join(ROOT, "tests", "merge_quotient_check.c"), "-o", exe, "-lm"])
    per = "200000" if os.environ.get("SYLBER_EXHAUSTIVE") == "1" else "2000"
    out = subprocess.run([exe, per], capture_output=True, text=True)
    n, bad, first_bad = (int(x) for x in out.stdout.split())
    assert out.returncode == 0 and bad == 0 and first_bad == 0 and n >= 9878 * (5 * int(per) + 6), out.stdout
