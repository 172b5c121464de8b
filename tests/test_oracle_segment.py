"""Oracle pinning, CPU only: oracle/segment_ref.c against the golden get_segment vectors that
tools/gen_golden.py produced by running the reference (sylber/utils/segment_utils.py:72-131)."""
import os

import numpy as np
import pytest

from oracle import segment_oracle
from sylber_amd.synth_states import syllable_states


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "segment_cases.npz"))


def test_np_sum_order_matches_numpy():
    rng = np.random.default_rng(0)
    for n in list(range(0, 200)) + [384, 768, 769, 1000, 2999]:
        a = (rng.standard_normal(n) * 10).astype(np.float32)
        assert segment_oracle.np_sum(a) == a.sum(), n


def test_scalar_pow_is_libm_powf():
    rng = np.random.default_rng(1)
    v = rng.uniform(1e-3, 1e3, 20000).astype(np.float32)
    for x in v:
        assert segment_oracle.powf_half(x) == x ** .5


def test_oracle_matches_reference_goldens(cases):
    off = cases["offsets"]
    n_checked = 0
    for i in range(len(cases["T"])):
        if int(cases["T"][i]) > 499 and i % 3:
            continue  # keep the CPU suite quick; all 2999-frame cases run in the gpu tier
        st = syllable_states(int(cases["T"][i]), int(cases["seed"][i]), mode=str(cases["mode"][i]))
        got = segment_oracle.get_segment(st, float(cases["norm_thr"][i]), float(cases["merge_thr"][i]))
        exp = cases["segments"][off[i]:off[i + 1]]
        if len(exp) == 0:
            assert got.shape == (0,) and got.dtype == np.float64
        else:
            assert got.dtype == np.int64 and np.array_equal(got, exp), i
            feats = segment_oracle.mean_pool(st, got)
            assert np.isclose(np.nan_to_num(feats).astype(np.float64).sum(), cases["feat_sum"][i], rtol=0, atol=1e-6)
        n_checked += 1
    assert n_checked > 600


def test_mean_pool_is_sequential_row_sum():
    st = syllable_states(143, 5)
    seg = np.array([[0, 1], [3, 20], [20, 143]], dtype=np.int64)
    exp = np.stack([st[s:e].mean(0) for s, e in seg])
    assert np.array_equal(segment_oracle.mean_pool(st, seg), exp)


def test_edge_cases_shapes():
    z = np.zeros((10, 768), dtype=np.float32)
    r = segment_oracle.get_segment(z, 2.6, 0.8)
    assert r.shape == (0,)
    one = np.ones((1, 768), dtype=np.float32)
    r = segment_oracle.get_segment(one, 2.6, 0.8)
    assert np.array_equal(r, np.array([[0, 1]]))


def test_oracle_vs_reference_seeded_states(golden_dir):
    """the reference's own get_segment on 40 seeded state sequences, stored by tools/gen_golden_seeded_segment.py"""
    g = np.load(os.path.join(golden_dir, "segment_seeded.npz"))
    off = g["offsets"]
    assert len(g["seed"]) == 40
    for i in range(len(g["seed"])):
        st = syllable_states(int(g["T"][i]), int(g["seed"][i]), mode=str(g["mode"][i]))
        assert st.astype(np.float64).sum() == g["state_sum"][i], i   # the inputs the reference saw
        o = segment_oracle.get_segment(st, 2.6, 0.8)
        exp = g["segments"][off[i]:off[i + 1]]
        assert o.dtype == np.int64 and np.array_equal(o, exp), i


# ---- decision edges: ties, non-finite inputs, full tables (tests/segment_edge_cases.py, tools/gen_golden_segment_edges.py) ----
@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(os.path.join(golden_dir, "segment_edges.npz"))


def test_edge_golden_lists_the_builders_cases(edges):
    """the golden file holds every fixed case of the builder, in its order, at the builder's thresholds bit for bit, then the merge ties in
    threes (v, one ulp above, one ulp below) on the builder's tie clips"""
    import segment_edge_cases as E
    fixed = E.fixed_cases()
    n = len(fixed)
    assert [str(x) for x in edges["name"][:n]] == [c[1] for c in fixed] and [str(x) for x in edges["clip"][:n]] == [c[2] for c in fixed]
    assert [str(x) for x in edges["family"][:n]] == [c[0] for c in fixed]
    assert [int(x) for x in edges["norm_bits"][:n]] == [E.f32_bits(c[3]) for c in fixed]
    assert [int(x) for x in edges["merge_bits"][:n]] == [E.f32_bits(c[4]) for c in fixed]
    fam = [str(x) for x in edges["family"]]
    assert {f: fam.count(f) for f in set(fam)} == {"threshold_extremes": 24, "maximal_tables": 13, "non_finite": 33, "equal_values": 18,
                                                   "norm_ties": 27, "long_divisors": 2, "merge_ties": 537}
    assert all(f == "merge_ties" for f in fam[n:]) and (len(fam) - n) % 3 == 0
    mb = edges["merge_bits"][n:].view(np.float32).reshape(-1, 3)
    assert np.array_equal(np.nextafter(mb[:, 0], np.float32(np.inf)), mb[:, 1]) and np.array_equal(np.nextafter(mb[:, 0], np.float32(-np.inf)), mb[:, 2])
    assert set(str(x) for x in edges["clip"][n:]) == set(E.TIE_CLIPS) and (edges["norm_bits"][n:] == E.f32_bits(E.NORM_THR)).all()
    ph = edges["tie_phase"][n::3]
    assert (ph == 1).sum() == 144 and (ph == 2).sum() == 35 and int(edges["tie_differs"][n::3].sum()) == 99


def test_oracle_matches_reference_edge_goldens(edges):
    """oracle == the reference's table on every edge case, on the input the reference saw (NaN-aware checksum); and every merge-tie triple
    still makes its tie comparison: the trace of the run at v holds v, with the recorded phase and frame"""
    import segment_edge_cases as E
    off = edges["offsets"]
    clips = {}
    for i in range(len(edges["name"])):
        clip = str(edges["clip"][i])
        if clip not in clips:
            clips[clip] = E.build_clip(clip)
            s, nf = E.checksum(clips[clip])
            assert s == edges["state_sum"][i] and nf == edges["state_nonfinite"][i], clip
        st = clips[clip]
        nt, mt = E.bits_f32(edges["norm_bits"][i]), E.bits_f32(edges["merge_bits"][i])
        exp = edges["segments"][off[i]:off[i + 1]]
        if edges["tie_phase"][i] and str(edges["name"][i]).endswith("_0"):
            got, val, phase, frame = segment_oracle.get_segment_trace(st, nt, mt)
            k = np.flatnonzero(val.view(np.uint32) == edges["merge_bits"][i])
            assert len(k) and phase[k[0]] == edges["tie_phase"][i] and frame[k[0]] == edges["tie_frame"][i], edges["name"][i]
        else:
            got = segment_oracle.get_segment(st, nt, mt)
        assert len(got) == len(exp) and np.array_equal(got.reshape(-1, 2), exp), edges["name"][i]
    # the maximal tables are maximal: nseg == T where nothing merges, ceil(T / 2) runs of one frame under alternation
    tab = {str(n): off[i + 1] - off[i] for i, n in enumerate(edges["name"])}
    assert tab["allspeech_T513@merge1.5"] == 513 and tab["allspeech_T512@merge1.5"] == 512 and tab["even_T513"] == 257 and tab["odd_T513"] == 256
    assert tab["loud_T8400@merge-2"] == 1                    # one run, one segment: the merge update divides by every count up to 8400


@pytest.mark.reference
def test_edge_goldens_regenerate_from_the_reference(edges):
    """every fixed case and every 4th merge-tie triple regenerated live from the reference's own get_segment (needs the upstream checkout)"""
    from tools import ref_shim
    if not ref_shim.available():
        pytest.skip("reference checkout not present")
    import warnings
    import segment_edge_cases as E
    _, seg_utils, _ = ref_shim.load()
    off, n = edges["offsets"], len(E.fixed_cases())
    pick = list(range(n)) + [i for i in range(n, len(edges["name"])) if ((i - n) // 3) % 4 == 0]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i in pick:
            st = E.build_clip(str(edges["clip"][i]))
            r = seg_utils.get_segment(st, float(E.bits_f32(edges["norm_bits"][i])), float(E.bits_f32(edges["merge_bits"][i])))
            assert np.array_equal(np.asarray(r).reshape(-1, 2), edges["segments"][off[i]:off[i + 1]]), edges["name"][i]
