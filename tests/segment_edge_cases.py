"""Inputs of the segmenter's edge-case goldens (tests/golden/segment_edges.npz, written by tools/gen_golden_segment_edges.py): a
deterministic builder  clip name -> states float32 [T, 768]  and the list of fixed cases  (name, clip, norm_thr, merge_thr).  The golden
file stores no inputs, only each case's clip name, its thresholds as float32 bit patterns, the reference's segment table and a checksum of
the input; the merge-tie cases (thresholds that ARE one of the similarities a clip produces, and their float32 neighbours) exist only in
the golden file, on the clips of ``TIE_CLIPS``.  No reference code here: clips are seeded ``syllable_states`` sequences and plain edits of them.

Clip names:  <kind>_T<frames>[_s<seed>]
  allspeech / normal   ``syllable_states`` of that mode (seed 7100 + s / 7200 + s)
  loud                 allspeech scaled by 1.5: every frame norm above 2.6 (allspeech itself has a quiet frame now and then), ONE run of speech
  zero                 all zeros
  even / odd           an allspeech clip with every odd / even frame zeroed: speech on even / odd frames only, ceil(T / 2) or T // 2 runs of one frame
  nanmid / infmid      allspeech, one NaN / +Inf element (frame T // 2, dimension 300)
  nanfirst / nanlast   allspeech, one NaN element in frame 0 / frame T - 1
  big4                 allspeech, frames T // 3 .. T // 3 + 3 scaled by 1e19: the squared sums overflow to +Inf
  tiny16 / tiny20 / tiny30   allspeech scaled by 1e-16 / 1e-20 / 1e-30: squared sums far below the 1e-8 floor, so every similarity is ~0 and
                       nothing merges at 0.8; run at merge_thr = -2 as well, where everything merges and the merge update sees tiny
                       dividends (1e-30: below 2^-100, the plain-division fallback on every lane)
  halfzero             allspeech with every dimension >= 384 zeroed (zero merge dividends on half of a wave's lanes)
  dup7                 an allspeech clip of ceil(T / 7) frames, every frame repeated 7 times (equal sweep values: first-maximum argmax)
  const                one frame repeated T times
  const2               one frame repeated T // 2 times, then another one
  mirror               allspeech whose second half is its first half reversed
"""
import numpy as np

from sylber_amd.synth_states import syllable_states

D = 768
SIZES = (64, 257, 513)            # 513 crosses the wide path's LDS limit for one run (512 frames)
NORM_THR, MERGE_THR = 2.6, 0.8    # the product's defaults
TIE_CLIPS = ["normal_T%d_s%d" % (T, s) for T in (64, 257) for s in (0, 1, 2)]
LONG_T = 8400                     # merge divisors beyond 8192


def build_clip(name: str) -> np.ndarray:
    parts = name.split("_")
    kind, T = parts[0], int(parts[1][1:])
    s = int(parts[2][1:]) if len(parts) > 2 else 0
    if kind == "normal":
        return syllable_states(T, 7200 + s, mode="normal")
    if kind == "zero":
        return np.zeros((T, D), dtype=np.float32)
    if kind == "dup7":
        return np.ascontiguousarray(np.repeat(syllable_states((T + 6) // 7, 7100 + s, mode="allspeech"), 7, axis=0)[:T])
    st = syllable_states(T, 7100 + s, mode="allspeech").copy()
    if kind == "allspeech":
        pass
    elif kind == "loud":
        st *= np.float32(1.5)
    elif kind == "even":
        st[1::2] = 0
    elif kind == "odd":
        st[0::2] = 0
    elif kind == "nanmid":
        st[T // 2, 300] = np.nan
    elif kind == "infmid":
        st[T // 2, 300] = np.inf
    elif kind == "nanfirst":
        st[0, 300] = np.nan
    elif kind == "nanlast":
        st[T - 1, 300] = np.nan
    elif kind == "big4":
        st[T // 3:T // 3 + 4] *= np.float32(1e19)
    elif kind == "tiny16":
        st *= np.float32(1e-16)
    elif kind == "tiny20":
        st *= np.float32(1e-20)
    elif kind == "tiny30":
        st *= np.float32(1e-30)
    elif kind == "halfzero":
        st[:, 384:] = 0
    elif kind == "const":
        st[:] = st[0]
    elif kind == "const2":
        st[:T // 2] = st[0]
        st[T // 2:] = st[T - 1]
    elif kind == "mirror":
        h = T // 2
        st[T - h:] = st[:h][::-1]
    else:
        raise ValueError("unknown clip %r" % name)
    return np.ascontiguousarray(st, dtype=np.float32)


def frame_norms(st: np.ndarray) -> np.ndarray:
    """float32 frame norms as get_segment's array path evaluates them: pairwise row sums of the squares, + 1e-8, correctly rounded sqrt"""
    with np.errstate(all="ignore"):
        return ((st ** 2).sum(-1) + np.float32(1e-8)) ** np.float32(.5)


def _norm_tie_thresholds(clip: str):
    """the norm of the clip's median-norm frame and its two float32 neighbours: that frame is speech at -1 and 0 ulp and silence at +1"""
    n = frame_norms(build_clip(clip))
    v = np.sort(n)[len(n) // 2]
    return [("m1", np.nextafter(v, np.float32(-np.inf))), ("0", v), ("p1", np.nextafter(v, np.float32(np.inf)))]


def fixed_cases():
    """[(family, case name, clip name, norm_thr float32, merge_thr float32)]: every case whose thresholds do not come out of a reference run"""
    f32 = np.float32
    out = []
    for T in SIZES:
        for mt in (1.5, 1.0, 0.0, -2.0):
            out.append(("threshold_extremes", "allspeech_T%d@merge%g" % (T, mt), "allspeech_T%d" % T, f32(NORM_THR), f32(mt)))
        for nt in (0.0, -1.0):
            for clip in ("normal_T%d_s3" % T, "zero_T%d" % T):
                out.append(("threshold_extremes", "%s@norm%g" % (clip, nt), clip, f32(nt), f32(MERGE_THR)))
    for T in SIZES:
        for L in (T, T - 1):
            for kind in ("even", "odd"):
                out.append(("maximal_tables", "%s_T%d" % (kind, L), "%s_T%d" % (kind, L), f32(NORM_THR), f32(MERGE_THR)))
    out.append(("maximal_tables", "allspeech_T512@merge1.5", "allspeech_T512", f32(NORM_THR), f32(1.5)))   # (513: under threshold_extremes)
    for T in SIZES:
        for kind in ("nanmid", "infmid", "nanfirst", "nanlast", "big4", "halfzero"):
            out.append(("non_finite", "%s_T%d" % (kind, T), "%s_T%d" % (kind, T), f32(NORM_THR), f32(MERGE_THR)))
        for kind in ("tiny16", "tiny20"):
            out.append(("non_finite", "%s_T%d@norm0" % (kind, T), "%s_T%d" % (kind, T), f32(0.0), f32(MERGE_THR)))
        for kind in ("tiny16", "tiny20", "tiny30"):
            out.append(("non_finite", "%s_T%d@norm0,merge-2" % (kind, T), "%s_T%d" % (kind, T), f32(0.0), f32(-2.0)))
    for T in SIZES:
        for kind, mts in (("dup7", (0.8, 0.95)), ("const", (0.8, 1.0)), ("const2", (0.8,)), ("mirror", (0.8,))):
            for mt in mts:
                out.append(("equal_values", "%s_T%d@merge%g" % (kind, T, mt), "%s_T%d" % (kind, T), f32(NORM_THR), f32(mt)))
    for T in SIZES:
        for s in (4, 5, 6):
            clip = "normal_T%d_s%d" % (T, s)
            for tag, nt in _norm_tie_thresholds(clip):
                out.append(("norm_ties", "%s@normtie%s" % (clip, tag), clip, nt, f32(MERGE_THR)))
    for mt in (-2.0, 0.8):
        out.append(("long_divisors", "loud_T%d@merge%g" % (LONG_T, mt), "loud_T%d" % LONG_T, f32(NORM_THR), f32(mt)))
    assert len({c[1] for c in out}) == len(out)
    return out


def checksum(st: np.ndarray):
    """(float64 sum of the finite part, count of non-finite elements) of an input"""
    return float(np.nan_to_num(st.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0).sum()), int((~np.isfinite(st)).sum())


def f32_bits(v) -> int:
    return int(np.asarray(v, dtype=np.float32).view(np.uint32))


def bits_f32(u) -> np.float32:
    return np.asarray(u, dtype=np.uint32).view(np.float32)[()]
