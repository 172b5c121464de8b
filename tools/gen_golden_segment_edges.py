"""Golden vectors for the segmenter's decision edges (survey container only): the REFERENCE's own ``get_segment``
(sylber/utils/segment_utils.py:72-131) on the cases of tests/segment_edge_cases.py, stored in tests/golden/segment_edges.npz and read by
tests/test_oracle_segment.py (CPU) and tests/test_gpu_segment_edges.py (every GPU path).  Contains no reference code; never runs on the
GPU box.  The oracle (oracle/segment_ref.c) must agree with the reference bit for bit on every case before anything is written.

Fixed cases (``segment_edge_cases.fixed_cases``): threshold extremes, maximal tables, non-finite and extreme magnitudes, equal values,
norm ties, long divisors.  The reference raised on none of them, so none was dropped.

Merge ties are made here, because they need the values the reference's arithmetic produces: for each clip of ``TIE_CLIPS`` the oracle's
trace at 0.8 lists every value compared with ``merge_thr``; per phase (1 = greedy scan, 2 = re-merge) the 24 values nearest 0.8 that pass
the check below are taken (fewer where a clip has fewer; phase 2 also draws on runs at other thresholds, see ``phase2_candidates``), and
each value v becomes three cases, merge_thr = v, nextafter(v, +inf), nextafter(v, -inf).  A changed
threshold changes the run, so a triple is kept only if, in the traces of the NEW runs at v and at nextafter(v, +inf), the same comparison
(same position, phase and frame, value == v bit for bit, identical traces before it) is still made: it is then decided `merge` at v and
`split` one ulp above.  A candidate that fails this proves nothing and is not stored; every stored triple is asserted to pass.

File: name / family / clip [n] strings, norm_bits / merge_bits [n] uint32 (float32 bit patterns), offsets [n + 1] and segments [sum, 2] int32
(the flattened tables), state_sum [n] float64 and state_nonfinite [n] (``segment_edge_cases.checksum`` of the input), tie_phase / tie_frame
[n] (0 / -1 outside the merge-tie family), tie_differs [n] (1 where the table at v differs from the table one ulp above).

    python tools/gen_golden_segment_edges.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segment_edge_cases as E                            # noqa: E402
from oracle import segment_oracle                         # noqa: E402
from tools import ref_shim                                # noqa: E402

TIES_PER_PHASE = 24
GOLDEN = os.path.join(ROOT, "tests", "golden", "segment_edges.npz")


def reference_table(seg_utils, st, nt, mt):
    """the reference's table at exactly these float32 thresholds, and the oracle's, which must be the same"""
    r = seg_utils.get_segment(st, float(nt), float(mt))
    o = segment_oracle.get_segment(st, nt, mt)
    assert r.shape == o.shape and np.array_equal(r, o), "the oracle disagrees with the reference"
    return np.asarray(r).reshape(-1, 2).astype(np.int32)


def tie_still_decided(st, nt, v):
    """True if the runs at merge_thr = v and one ulp above both make the comparison of value v, at the same place, after identical
    traces: the first decision on which they differ is then `v >= v` against `v >= nextafter(v)`"""
    up = np.nextafter(v, np.float32(np.inf))
    _, va, pa, fa = segment_oracle.get_segment_trace(st, nt, v)
    _, vb, pb, fb = segment_oracle.get_segment_trace(st, nt, up)
    ia, ib = np.flatnonzero(va.view(np.uint32) == v.view(np.uint32)), np.flatnonzero(vb.view(np.uint32) == v.view(np.uint32))
    if len(ia) == 0 or len(ib) == 0 or ia[0] != ib[0]:
        return None
    k = int(ia[0])
    same = (np.array_equal(va[:k + 1].view(np.uint32), vb[:k + 1].view(np.uint32)) and np.array_equal(pa[:k + 1], pb[:k + 1])
            and np.array_equal(fa[:k + 1], fb[:k + 1]))
    if not same or not (va[k] >= v) or (vb[k] >= up):
        return None
    return int(pa[k]), int(fa[k])


def phase2_candidates(st, nt):
    """Re-merge similarities of runs at OTHER thresholds.  A phase-2 value of the run at 0.8 rarely survives as its own threshold: where both
    segments are single frames it equals the scan's similarity at that frame bit for bit (a phase-1 tie, taken there), and elsewhere the
    changed threshold moves the segments its centroids are means of.  So the runs at 0.5, 0.501 .. 0.989 are traced as well and the two
    re-merge values nearest each run's own threshold offered: close to it few scan decisions change, and the value tends to be made again."""
    out = []
    for t in np.arange(0.5, 0.99, 0.001):
        _, va, pa, _ = segment_oracle.get_segment_trace(st, nt, np.float32(t))
        p2 = np.unique(va[(pa == 2) & np.isfinite(va)])
        out.extend(p2[np.argsort(np.abs(p2.astype(np.float64) - t), kind="stable")][:2])
    return np.unique(np.array(out, dtype=np.float32))


def merge_tie_cases(seg_utils):
    """[(name, clip, nt, mt, phase, frame, differs)] in threes: v, one ulp above, one ulp below"""
    out, dropped = [], 0
    nt = np.float32(E.NORM_THR)
    for clip in E.TIE_CLIPS:
        st = E.build_clip(clip)
        _, val, phase, frame = segment_oracle.get_segment_trace(st, nt, np.float32(E.MERGE_THR))
        seen = set()
        for ph in (1, 2):
            cand = np.unique(val[(phase == ph) & np.isfinite(val)])
            if ph == 2:
                cand = np.concatenate([cand, phase2_candidates(st, nt)])
            cand = cand[np.argsort(np.abs(cand.astype(np.float64) - E.MERGE_THR), kind="stable")]
            kept = 0
            for v in cand:
                if kept == TIES_PER_PHASE:
                    break
                v = np.float32(v)
                hit = tie_still_decided(st, nt, v)
                if hit is None or hit[0] != ph or E.f32_bits(v) in seen:
                    dropped += 1
                    continue
                seen.add(E.f32_bits(v))
                kept += 1
                up, dn = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
                tabs = [reference_table(seg_utils, st, nt, t) for t in (v, up, dn)]
                differs = int(not np.array_equal(tabs[0], tabs[1]))
                for tag, t, tab in zip(("0", "p1", "m1"), (v, up, dn), tabs):
                    out.append(("%s@mergetie_p%d_f%d_%08x_%s" % (clip, hit[0], hit[1], E.f32_bits(v), tag), clip, nt, t, hit[0], hit[1], differs, tab))
    # every stored triple flips where it must (asserted on the traces of the runs at the stored thresholds)
    for i in range(0, len(out), 3):
        st = E.build_clip(out[i][1])
        assert tie_still_decided(st, nt, out[i][3]) == (out[i][4], out[i][5]), out[i][0]
        assert out[i + 1][3] == np.nextafter(out[i][3], np.float32(np.inf)) and out[i + 2][3] == np.nextafter(out[i][3], np.float32(-np.inf))
    return out, dropped


def main():
    _, seg_utils, _ = ref_shim.load()
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    rows = []
    for family, name, clip, nt, mt in E.fixed_cases():
        st = E.build_clip(clip)
        rows.append((family, name, clip, nt, mt, 0, -1, 0, reference_table(seg_utils, st, nt, mt)))
    ties, dropped = merge_tie_cases(seg_utils)
    for name, clip, nt, mt, ph, fr, differs, tab in ties:
        rows.append(("merge_ties", name, clip, nt, mt, ph, fr, differs, tab))
    assert len({r[1] for r in rows}) == len(rows)
    sums = {}
    for r in rows:
        if r[2] not in sums:
            sums[r[2]] = E.checksum(E.build_clip(r[2]))
    offs = np.concatenate([[0], np.cumsum([len(r[8]) for r in rows])]).astype(np.int32)
    np.savez_compressed(
        GOLDEN, name=np.array([r[1] for r in rows]), family=np.array([r[0] for r in rows]), clip=np.array([r[2] for r in rows]),
        norm_bits=np.array([E.f32_bits(r[3]) for r in rows], dtype=np.uint32), merge_bits=np.array([E.f32_bits(r[4]) for r in rows], dtype=np.uint32),
        offsets=offs, segments=np.concatenate([r[8] for r in rows], 0).astype(np.int32),
        state_sum=np.array([sums[r[2]][0] for r in rows]), state_nonfinite=np.array([sums[r[2]][1] for r in rows], dtype=np.int32),
        tie_phase=np.array([r[5] for r in rows], dtype=np.int8), tie_frame=np.array([r[6] for r in rows], dtype=np.int32),
        tie_differs=np.array([r[7] for r in rows], dtype=np.int8))
    fam = {}
    for r in rows:
        fam[r[0]] = fam.get(r[0], 0) + 1
    nt3 = len(ties) // 3
    print("wrote tests/golden/segment_edges.npz: %d cases %s, %d segments, %d bytes" % (len(rows), fam, offs[-1], os.path.getsize(GOLDEN)))
    print("merge ties: %d tie decisions (phase 1: %d, phase 2: %d), %d candidates dropped, tables differ across the tie in %d" % (
        nt3, sum(1 for t in ties[::3] if t[4] == 1), sum(1 for t in ties[::3] if t[4] == 2), dropped, sum(t[6] for t in ties[::3])))


if __name__ == "__main__":
    main()
