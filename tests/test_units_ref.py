"""CPU tier, syllable units: the fixture of the reference's own ``expand_feature`` / ``resynthesize(features=...)`` on decoded units
(tests/golden/units.npz, written by tools/gen_golden_units.py) against the float64 restatement tests/units_ref.py, the equivalence
of upstream's duration layout and the span layout the C-ABI takes, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

import units_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "units.npz"))


def test_fixture_cases(gold):
    """the fixture holds what its generator promises: a near-zero unit, a leading gap, adjacent units"""
    c1, c2, units, spans, n = gold["c1"], gold["c2"], gold["units"], gold["spans"], gold["nunits"]
    assert c1.shape == (64, 768) and c2.shape == (32, 768)
    dec = U.decode(units, [c1, c2])
    norms = np.sqrt((dec.astype(np.float64) ** 2).sum(-1))
    assert any(norms[b, j] < 1e-4 for b in range(2) for j in range(n[b]))
    assert spans[0, 0, 0] > 0 and gold["durations2"][0, 0, 1] == 0
    assert any(spans[b, j, 1] == spans[b, j + 1, 0] for b in range(2) for j in range(n[b] - 1))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "units.npz")) < 1 << 20


def test_reference_expansion_matches_restatement(gold):
    """the reference's expand_feature output == the restatement of both layouts, exactly (it only copies rows)"""
    T = int(gold["T"])
    feats = U.decode(gold["units"], [gold["c1"], gold["c2"]])
    avg, dur = U.spans_to_durations(feats, gold["spans"], gold["nunits"], T)
    assert np.array_equal(dur, gold["durations2"])
    assert np.array_equal(U.expand_feature(avg, dur), gold["expanded2"])
    assert np.array_equal(U.expand_spans(feats, gold["spans"], gold["nunits"], T), gold["expanded2"])


def test_duration_layout_equals_span_layout():
    """for random span tables (gaps, no gaps, a leading gap, a unit at the last frame) the two layouts agree"""
    rng = np.random.default_rng(3)
    for _ in range(50):
        T, B, S = int(rng.integers(5, 80)), 3, 6
        spans = np.zeros((B, S, 2), np.int64)
        n = np.zeros(B, np.int64)
        for b in range(B):
            t = int(rng.integers(0, 3))
            while n[b] < S and t < T:
                e = min(T, t + int(rng.integers(1, 6)))
                spans[b, n[b]] = (t, e)
                n[b] += 1
                t = e + int(rng.integers(0, 3))
        feats = rng.standard_normal((B, S, 8)).astype(np.float32)
        avg, dur = U.spans_to_durations(feats, spans, n, T)
        assert (dur.sum((1, 2)) == T).all()
        assert np.array_equal(U.expand_feature(avg, dur), U.expand_spans(feats, spans, n, T))


def test_residual_restatement_recovers_known_ids(gold):
    ids, d1, d2 = U.residual_assign(gold["tokens"], gold["c1"], gold["c2"])
    assert np.array_equal(ids, gold["tok_ids"])
    dec = U.decode(ids, [gold["c1"], gold["c2"]])
    assert np.array_equal(dec, gold["c1"][ids[:, 0]] + gold["c2"][ids[:, 1]])


def test_header_declares_the_unit_path():
    with open(os.path.join(ROOT, "include", "sylber_hip.h")) as f:
        h = f.read()
    for pat in (r"int64_t sylber_km_residual_workspace_floats\(int32_t n, int32_t K1, int32_t K2, int32_t D\);",
                r"int sylber_km_assign_residual\(const float\* feats_dev, int32_t n, const float\* c1_dev, int32_t K1, const float\* c2_dev,",
                r"int sylber_km_decode_residual\(const int32_t\* idx_dev, int32_t n, const float\* c1_dev, int32_t K1,",
                r"int64_t sylber_condition_units_workspace_floats\(sylber_mlp_t m, int32_t B, int32_t S\);",
                r"int sylber_condition_units\(sylber_mlp_t m, const float\* c1_dev, int32_t K1, const float\* c2_dev, int32_t K2,",
                r"int sylber_expand_units\(const float\* feats_dev, const int32_t\* durations_dev, int32_t B, int32_t S, int32_t D,"):
        assert re.search(pat, h), pat


def test_library_exports_the_unit_path():
    from sylber_amd import _lib
    lib = _lib.load()
    for name in ("sylber_km_assign_residual", "sylber_km_decode_residual", "sylber_km_residual_workspace_floats",
                 "sylber_condition_units", "sylber_condition_units_workspace_floats", "sylber_expand_units"):
        assert hasattr(lib, name), name
    assert lib.sylber_km_residual_workspace_floats(0, 64, 32, 768) == -1
    assert lib.sylber_km_residual_workspace_floats(10, 64, 32, 768) > 10 * 768


def test_public_names():
    import sylber_amd
    from sylber_amd import downstream
    for name in ("ResidualKMQuantizer", "expand_feature", "load_km_quantizer", "load_residualkm_quantizer"):
        assert getattr(sylber_amd, name) is getattr(downstream, name)
    from sylber_amd import SegmentSynthesis
    assert callable(SegmentSynthesis.tokenize) and callable(SegmentSynthesis.synthesize_units)
