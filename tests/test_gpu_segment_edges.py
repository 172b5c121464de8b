"""GPU tier: the segmenter at its decision edges.  Every case of tests/golden/segment_edges.npz (the reference's own get_segment on the
inputs of tests/segment_edge_cases.py: threshold extremes, maximal tables, non-finite and extreme magnitudes, equal values, norm ties,
merge ties at -1 / 0 / +1 ulp, merge divisors beyond 8192) must come out of EVERY GPU path bit for bit -- nseg, the table, and the pooled
features against the oracle's mean-pool -- and the scalar chain behind the `>=` decisions (the device's glibc-powf restatement, sqrtf, the
IEEE division, the one-division merge quotient) must equal the host's for ~5e7 inputs.  No tolerances, no case excused.

Paths: sylber_segment wide; sylber_segment one workgroup per utterance (SYLBER_OPT_SEGMENT = -1); sylber_segment_frames with the clip in
a longer row whose tail is NaN, and one whose tail is loud speech; sylber_segment_packed with the clip as the middle of three clips.

Wall time of this file on an MI355X: 5.6 s for its 13 tests, encoder set-up and the host references included (slowest: the merge-quotient
test 0.7 s, the fixed cases on the wide path 0.4 s, the 537 tie launches of one path 0.2 s)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import segment_edge_cases as E
from oracle import segment_oracle

pytestmark = pytest.mark.gpu

PATHS = ["wide", "per_utterance", "frames_nan_tail", "frames_loud_tail", "packed"]
TAIL = 41                                   # rows behind the clip in the padded paths (an odd count: the row pitch is no multiple of anything)


@pytest.fixture(scope="module")
def enc():
    from sylber_amd import HubertEncoderHIP
    from sylber_amd.weights import synthetic_state_dict
    return HubertEncoderHIP(synthetic_state_dict(0, num_layers=1), num_layers=1)


class Cases:
    """the golden file's cases, the clips they run on (built once, never modified) and the expected pooled features (oracle mean-pool of
    the golden table, once per case)"""

    def __init__(self, golden_dir):
        g = np.load(os.path.join(golden_dir, "segment_edges.npz"))
        self.name = [str(x) for x in g["name"]]
        self.family = [str(x) for x in g["family"]]
        self.clip = [str(x) for x in g["clip"]]
        self.nt = g["norm_bits"].view(np.float32)
        self.mt = g["merge_bits"].view(np.float32)
        self.off = g["offsets"]
        self.seg = g["segments"].astype(np.int64)
        self._clips, self._feats = {}, {}
        self.loud = (E.build_clip("allspeech_T%d" % (max(E.SIZES) + TAIL)) * np.float32(2)).astype(np.float32)   # every frame above 2.6

    def __len__(self):
        return len(self.name)

    def states(self, i):
        c = self.clip[i]
        if c not in self._clips:
            self._clips[c] = E.build_clip(c)
            self._clips[c].setflags(write=False)
        return self._clips[c]

    def table(self, i):
        return self.seg[self.off[i]:self.off[i + 1]]

    def feats(self, i):
        if i not in self._feats:
            with np.errstate(all="ignore"):
                self._feats[i] = segment_oracle.mean_pool(self.states(i), self.table(i))
        return self._feats[i]

    def check(self, i, path, seg_row, nseg, feat_row):
        exp = self.table(i)
        what = (self.name[i], path)
        assert int(nseg) == len(exp), what + (int(nseg), len(exp))
        assert np.array_equal(seg_row[:len(exp)], exp), what
        if len(exp):
            assert np.array_equal(feat_row[:len(exp)], self.feats(i), equal_nan=True), what


@pytest.fixture(scope="module")
def cases(golden_dir):
    return Cases(golden_dir)


def _samples(T):
    """a sample count that has exactly T frames (400-sample window, hop 320)"""
    return 400 + 320 * (T - 1)


def _stage(cases, idx, path, dev):
    """the input tensor(s) of one launch of `path` over the cases idx (all of one T for the unpadded paths): (kind, hidden, extra)"""
    sts = [cases.states(i) for i in idx]
    if path in ("wide", "per_utterance"):
        assert len({len(s) for s in sts}) == 1
        return torch.from_numpy(np.stack(sts)).to(dev), None
    if path.startswith("frames"):
        Tp = max(len(s) for s in sts) + TAIL
        h = np.full((len(sts), Tp, E.D), np.nan, dtype=np.float32) if path == "frames_nan_tail" else np.ascontiguousarray(
            np.broadcast_to(cases.loud[:Tp], (len(sts), Tp, E.D))).copy()
        for b, s in enumerate(sts):
            h[b, :len(s)] = s
        return torch.from_numpy(h).to(dev), [len(s) for s in sts]
    # packed: [filler, clip, filler] per case; slot slack (rows behind a clip's own frames) is NaN
    from sylber_amd.segmenter import packed_layout
    fill_a, fill_b = cases.loud[:5], cases.loud[7:20]
    clips = []
    for s in sts:
        clips += [fill_a, s, fill_b]
    lengths = [_samples(len(c)) for c in clips]
    offsets, frames = packed_layout(lengths)
    assert [int(f) for f in frames] == [len(c) for c in clips]
    h = np.full((int(offsets[-1]), E.D), np.nan, dtype=np.float32)
    for c, o in zip(clips, offsets[:-1]):
        h[int(o):int(o) + len(c)] = c
    return torch.from_numpy(h).to(dev), (lengths, (offsets, frames))


def _launch(enc, path, hidden, extra, nt, mt):
    """one launch; returns host arrays (seg [n, K, 2], nseg [n], feats [n, K, 768]) with one row per CASE"""
    enc.set_option(9, -1 if path == "per_utterance" else 0)
    if path in ("wide", "per_utterance"):
        seg, nseg, feats = enc.segment(hidden, nt, mt)
    elif path.startswith("frames"):
        seg, nseg, feats = enc.segment(hidden, nt, mt, frames=extra)
    else:
        seg, nseg, feats = enc.segment_packed(hidden, extra[0], nt, mt, layout=extra[1])
        seg, nseg, feats = seg[1::3], nseg[1::3], feats[1::3]
    torch.cuda.synchronize()
    return seg.cpu().numpy(), nseg.cpu().numpy(), feats.cpu().numpy()


def _run_cases(enc, cases, idx, path):
    """the cases idx, batched: one launch per (thresholds) -- per (T, thresholds) on the unpadded paths"""
    groups = {}
    for i in idx:
        key = (E.f32_bits(cases.nt[i]), E.f32_bits(cases.mt[i])) + ((len(cases.states(i)),) if path in ("wide", "per_utterance") else ())
        groups.setdefault(key, []).append(i)
    for key, members in groups.items():
        hidden, extra = _stage(cases, members, path, enc.device)
        seg, nseg, feats = _launch(enc, path, hidden, extra, cases.nt[members[0]], cases.mt[members[0]])
        for j, i in enumerate(members):
            cases.check(i, path, seg[j], nseg[j], feats[j])
    return len(groups)


@pytest.mark.parametrize("path", PATHS)
def test_fixed_edge_cases_bit_exact(enc, cases, path):
    """every fixed case (all families but the merge ties) on `path`; the 8400-frame clips on the two sylber_segment paths only"""
    idx = [i for i in range(len(cases)) if cases.family[i] != "merge_ties"
           and (cases.family[i] != "long_divisors" or path in ("wide", "per_utterance"))]
    assert len(idx) == (117 if path in ("wide", "per_utterance") else 115)
    assert _run_cases(enc, cases, idx, path) > 30


@pytest.mark.parametrize("path", PATHS)
def test_merge_ties_bit_exact(enc, cases, path):
    """merge_thr IS one of the similarities the clip produces (scan: 144 decisions, re-merge: 35), and its two float32 neighbours: one launch
    per threshold on the clip's staged input.  A last-bit error anywhere in dot / powf(cc) / norm flips the decision at v or one ulp above."""
    idx = [i for i in range(len(cases)) if cases.family[i] == "merge_ties"]
    assert len(idx) == 537
    staged = {}
    for i in idx:
        c = cases.clip[i]
        if c not in staged:
            staged[c] = _stage(cases, [i], path, enc.device)
        seg, nseg, feats = _launch(enc, path, staged[c][0], staged[c][1], cases.nt[i], cases.mt[i])
        cases.check(i, path, seg[0], nseg[0], feats[0])


def test_poisoned_workspace_one_case_per_family(enc, cases):
    """nothing is read from the workspace before it is written: one case per family again after the slab was filled with NaN / 0x7F bytes"""
    from sylber_amd import _lib
    first = {}
    for i in range(len(cases)):
        first.setdefault(cases.family[i], i)
    assert len(first) == 7
    for byte in (0xFF, 0x7F):
        for path in PATHS:
            for fam, i in first.items():
                if fam == "long_divisors" and path not in ("wide", "per_utterance"):
                    continue
                _lib.check(enc.lib.sylber_debug_poison_workspace(enc.handle, byte), "poison")
                _run_cases(enc, cases, [i], path)


# ---- the scalar chain, directly (sylber_debug_segment_scalars: kernels inside segment.hip, built with its flags) ----
def _scalars(enc, x, d):
    from sylber_amd import _lib
    xd, dd = torch.from_numpy(x).to(enc.device), torch.from_numpy(d).to(enc.device)
    outs = [torch.empty_like(xd) for _ in range(3)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(enc.device):
        st = enc.lib.sylber_debug_segment_scalars(p(xd), p(dd), x.size, p(outs[0]), p(outs[1]), p(outs[2]), None, None, None, 0, None,
                                                  ctypes.c_void_p(torch.cuda.current_stream(enc.device).cuda_stream))
    _lib.check(st, "sylber_debug_segment_scalars")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _mismatches(got, exp):
    """elements whose bits differ (any NaN equals any NaN: payloads are not part of the contract)"""
    return int((~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)))).sum())


def _check_unary_binary(enc, x, d, what):
    pw, sq, dv = _scalars(enc, x, d)
    with np.errstate(all="ignore"):
        bad = (_mismatches(pw, segment_oracle.powf_half_array(x)), _mismatches(sq, np.sqrt(x)), _mismatches(dv, x / d))
    print("%s: %d inputs, mismatches powf %d sqrtf %d division %d" % ((what, x.size) + bad))
    assert bad == (0, 0, 0), what


def test_device_powf_sqrt_division_equal_the_host(enc):
    """the code hipcc emits from powf_half.h against libm's powf(x, .5f), device sqrtf and a / b against numpy float32 (IEEE), bit for bit:
    * every 128th positive float32 bit pattern from +0 to +Inf, subnormals included (1.67e7 values); divisors: the same values in another
      order, so quotients overflow, underflow and land on subnormals as well;
    * ALL 1.1e7 patterns of [2.6^2, 16): the squared norms of frames and centroids from the speech threshold (2.6) up to norm 4, where
      powf's argument lives whenever the scan compares a quiet-to-medium frame (louder ones sit in coarser binades the sweep covers at
      1 / 128 density); divisors: norms drawn from [2.6, 12];
    * quotients: ALL 1.68e6 patterns q of [0.75, 0.85], the similarities within 0.05 of the default merge threshold, each as
      a = RN(q b), b a norm from [2.6, 12], so that a / b lands on or next to q."""
    rng = np.random.default_rng(5)
    sweep = np.arange(0, 0x7F800001, 128, dtype=np.uint32)                  # (ends on +Inf = 0x7F800000)
    x = sweep.view(np.float32)
    _check_unary_binary(enc, x, np.ascontiguousarray(np.roll(x[::-1], 12345)), "sweep")
    band = np.arange(E.f32_bits(2.6 * 2.6), E.f32_bits(16.0), dtype=np.uint32).view(np.float32)
    _check_unary_binary(enc, band, rng.uniform(2.6, 12.0, band.size).astype(np.float32), "squared-norm band")
    q = np.arange(E.f32_bits(0.75), E.f32_bits(0.85) + 1, dtype=np.uint32).view(np.float32)
    b = rng.uniform(2.6, 12.0, q.size).astype(np.float32)
    _check_unary_binary(enc, q * b, b, "quotient band")


def _quotient_inputs():
    """(c, x float32 [W, 768], cnt int32 [W]): three waves per divisor c1 = cnt + 1 in {2..8192} + {8193, 8200 .. 19995}:
    wave 0 all-fast (every dividend inside [2^-100, 2^126]: activation-like values at a random scale);
    wave 1 mixed (the same, with 1..8 elements replaced by 0, -0, subnormals, values either side of 2^-100 and of 2^126, +-Inf, NaN:
           ONE such lane sends the whole wave down the plain division);
    wave 2 by divisor index mod 5: all dividends exactly at and just above 2^-100 (all-fast, at its edge) / just below 2^-100
           (all-fallback) / at and just below 2^126 (all-fast) / just above 2^126 (all-fallback) / zeros and subnormals (all-fallback).
    Where c = 0 the dividend c * cnt + x is x itself, so those elements sit exactly where they are put."""
    rng = np.random.default_rng(6)
    divs = np.concatenate([np.arange(2, 8193), np.arange(8193, 20001, 7)])
    nd = len(divs)
    W = 3 * nd
    cnt = np.repeat(divs - 1, 3).astype(np.int32)
    scale = np.exp2(rng.integers(-8, 9, size=(W, 1))).astype(np.float32)
    c = (rng.standard_normal((W, 768)).astype(np.float32) * scale)
    x = (rng.standard_normal((W, 768)).astype(np.float32) * scale)
    lo, hi = E.f32_bits(2.0 ** -100), E.f32_bits(2.0 ** 126)
    special = np.array([0, 0x80000000, 1, 0x007FFFFF, 0x80000400, lo - 1, lo, lo + 1, lo - 0x00800000, 0x80000000 | (lo - 1), hi - 1, hi, hi + 1,
                        hi + 0x00800000, 0x80000000 | (hi + 1), 0x7F800000, 0xFF800000, 0x7FC00000], dtype=np.uint32).view(np.float32)
    outside = special[(np.abs(special) < np.float32(2.0 ** -100)) | ~(np.abs(special) <= np.float32(2.0 ** 126))]
    assert len(outside) == len(special) - 4
    for k in range(nd):
        w = 3 * k + 1
        pos = rng.choice(768, size=int(rng.integers(1, 9)), replace=False)
        c[w, pos] = 0
        x[w, pos] = special[rng.integers(0, len(special), size=len(pos))]
        x[w, pos[0]] = outside[rng.integers(0, len(outside))]               # at least one lane that needs the division
        w = 3 * k + 2
        j = np.arange(768, dtype=np.uint32)
        sign = (rng.integers(0, 2, 768).astype(np.uint32) << 31)
        pat = [lo + j, lo - 1 - j, hi - j, hi + 1 + j, np.where(j % 3 == 0, 0, rng.integers(1, 0x00800000, 768)).astype(np.uint32)][k % 5]
        c[w] = 0
        x[w] = (pat.astype(np.uint32) | sign).view(np.float32)
    return c, x, cnt


def test_device_merge_quotient_equals_the_plain_division(enc):
    """the scan's merge update through its own function (one IEEE division + two FMA corrections, or the plain division where the wave-wide
    ballot says so) against numpy float32  (c * n + x) / (n + 1)  without fusion, bit for bit, for every divisor 2..8192 and every 7th up
    to 20000, on waves that are all-fast, all-fallback and mixed (_quotient_inputs)"""
    from sylber_amd import _lib
    c, x, cnt = _quotient_inputs()
    W = len(cnt)
    with np.errstate(all="ignore"):
        n = cnt.astype(np.float32)[:, None]
        a = c * n + x
        exp = a / (n + np.float32(1))
        fallback = (~(np.abs(a) >= np.float32(2.0 ** -100)) | ~(np.abs(a) <= np.float32(2.0 ** 126))).any(1)
    kinds = fallback.reshape(-1, 3)
    assert not kinds[:, 0].any() and kinds[:, 1].all()                     # all-fast / mixed waves are what they are meant to be
    assert np.array_equal(kinds[:, 2], np.isin(np.arange(len(kinds)) % 5, (1, 3, 4)))          # ... and so are the edge waves
    cd, xd, nd_ = (torch.from_numpy(t).to(enc.device) for t in (c, x, cnt))
    out = torch.empty_like(cd)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(enc.device):
        st = enc.lib.sylber_debug_segment_scalars(None, None, 0, None, None, None, p(cd), p(xd), p(nd_), W, p(out),
                                                  ctypes.c_void_p(torch.cuda.current_stream(enc.device).cuda_stream))
    _lib.check(st, "sylber_debug_segment_scalars")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = ~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)))
    print("merge quotient: %d waves (%d take the division), %d dividends, %d mismatches" % (W, int(fallback.sum()), got.size, int(bad.sum())))
    assert not bad.any(), "first bad divisors: %s" % (np.unique(cnt[bad.any(1)])[:10] + 1)
