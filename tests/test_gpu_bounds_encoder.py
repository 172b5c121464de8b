"""GPU tier, guard bands (tests/guarded_alloc.py) around what ``HubertEncoderHIP`` hands to sylber_forward, sylber_forward_packed,
sylber_packed_gather, sylber_segment, sylber_segment_frames and sylber_segment_packed: two encoder layers, synthetic weights.

Every case runs once plainly and once per fill byte (0xFF, 0x00) with the wrapper's allocations (``hidden``, the tap buffers at widths
512 .. 6144, ``seg`` / ``nseg`` / ``feats``, the gathered rows) and the device-resident inputs (waveform, hidden states) between
guards.  ``check()`` finds any byte written outside them -- the last layer's epilogue maps padded rows ``b Tp + t`` onto ``b T + t``
straight into the caller's ``hidden``, so a row ``t >= T`` of the LAST clip would land right behind it -- and the defined parts of
the results (the whole ``hidden`` of a padded batch, each clip's own rows of a packed one, rows ``[0, L_i)`` of a conv tap,
``seg[b, :nseg[b]]`` / ``feats[b, :nseg[b]]``) are bit-identical across the three runs.  No tolerances.

Entry points of include/sylber_hip.h that no guard-band file (this one, test_gpu_bounds_ops.py, _downstream.py, _search.py) runs
under guards, and why: sylber_set_graph_mode (a captured graph pins the pointers of its first call); sylber_workspace_bytes and the
partition of the handle-owned workspace behind sylber_forward (no caller-owned buffer: it would need library support);
sylber_get_profile, sylber_get_fp16_audit, sylber_flac_info / _decode, sylber_packed_layout, sylber_cfm_packed_layout, sylber_dtw_plan,
sylber_ivf_work_items and the sylber_debug_* aids (their outputs are host arrays); sylber_knn_splits, sylber_num_frames /
_padded_frames, sylber_ingest_num_frames, the create / destroy / set_* calls and sylber_last_error (no output buffer at all).
sylber_amd/dist.py is out of scope.

Findings: none -- no guard was dirty and no result moved with the fill on an MI355X."""
import numpy as np
import pytest
import torch

import conv_stack_ref as cr
from guarded_alloc import three_runs
from sylber_amd import _lib
from sylber_amd.synth_states import syllable_states

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16", "fp16", "mixed16", "split16", "fp32", "fp8"]
BATCHES = {"ragged": (65, (65, 64, 1)), "one": (1, (1,))}


def _samples(t):
    return 320 * t + 80


@pytest.fixture(scope="module")
def encoders():
    from sylber_amd import HubertEncoderHIP
    from sylber_amd.weights import synthetic_state_dict
    assert torch.cuda.is_available(), "gpu tier needs the MI355X"
    sd = synthetic_state_dict(0, num_layers=2)
    cache = {}

    def get(precision, segment=0):
        if (precision, segment) not in cache:
            e = HubertEncoderHIP(sd, num_layers=2, precision=precision)
            if segment:
                e.set_option(_lib.OPT_SEGMENT, segment)
            cache[(precision, segment)] = e
        return cache[(precision, segment)]
    return get


def _wave(batch):
    T, frames = BATCHES[batch]
    lens = [_samples(t) for t in frames]
    g = torch.Generator().manual_seed(T)
    wav = torch.randn(len(lens), _samples(T), generator=g) * 0.3
    for b, n in enumerate(lens):
        wav[b, n:] = 0
    return wav.cuda(), lens


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), what


def _stages(enc_layers=2):
    """(name, stop stage, rows of the result that the header defines: None = all, else conv layer i's L_i)"""
    out = [("full", 0, None), ("conv features", 1, None), ("encoder LayerNorm", 2, None)]
    out += [("layer %d" % l, 3 + l, None) for l in range(enc_layers)]
    out += [("conv0 tap", _lib.TAP_CONV0, 0)] + [("conv%d tap" % i, _lib.TAP_CONV(i), i) for i in range(1, 7)]
    out += [("projection tap", _lib.TAP_PROJ, None), ("pos-conv tap", _lib.TAP_POSCONV, None)]
    out += [("layer %d tap %d" % (l, k), _lib.TAP_LAYER(l, k), None) for l in range(enc_layers) for k in range(6)]
    return out


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_stages_and_taps(encoders, precision, batch):
    enc = encoders(precision)
    wav, lens = _wave(batch)
    T, frames = BATCHES[batch]
    L = cr.conv_rows(wav.shape[1])
    for name, stage, conv in _stages():
        def run(g):
            w = wav if g is None else g.guarded_copy(wav, "wav")
            return enc.forward(w, lens, stop_stage=stage)
        plain, guarded = three_runs(run)
        if stage <= -8 and stage > -1024:
            assert plain.shape == (len(lens), T, _lib.ltap_width(-stage % 8, precision)), name
        rows = slice(None) if conv is None else slice(0, L[conv])
        for g, out in guarded:
            assert g.covers(out) and g.handed_out(out.numel() * 4), (name, g.names())
            _same(out[:, rows], plain[:, rows], (precision, batch, name, "fill 0x%02X" % g.fill))


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_packed_forward_segment_gather(encoders, precision):
    from sylber_amd.segmenter import packed_layout
    enc = encoders(precision)
    lens = [400, 41000, 9000]
    gen = torch.Generator().manual_seed(9)
    clips = [torch.randn(n, generator=gen) * 0.3 for n in lens]
    offsets, frames = packed_layout(lens)
    norms = enc.forward_packed(clips)[0].norm(dim=-1)
    thr = float(norms[int(offsets[1]):int(offsets[1]) + int(frames[1])].median())      # half of the long clip's frames are speech

    def run(g):
        hidden, off, fr = enc.forward_packed(clips)                  # the staged waveform and hidden are the wrapper's allocations
        assert list(off) == list(offsets) and list(fr) == list(frames)
        seg, nseg, feats = enc.segment_packed(hidden, lens, thr, 0.8)
        seg2, nseg2, none = enc.segment_packed(hidden, lens, thr, 0.8, with_features=False)
        assert none is None
        rows = enc.gather_packed(hidden, lens)
        return hidden, seg, nseg, feats, seg2, nseg2, rows
    plain, guarded = three_runs(run)

    def defined(r):
        hidden, seg, nseg, feats, seg2, nseg2, rows = r
        n = nseg.tolist()
        out = [hidden[int(offsets[b]):int(offsets[b]) + int(frames[b])] for b in range(len(lens))] + [nseg, nseg2, rows]
        for b in range(len(lens)):
            out += [seg[b, :n[b]], feats[b, :n[b]], seg2[b, :n[b]]]
        return out
    want = defined(plain)
    assert sum(plain[2].tolist()) > 0
    for g, r in guarded:
        assert all(g.covers(t) for t in r), g.names()
        assert g.handed_out(int(offsets[-1]) * 768 * 4) and g.handed_out(int(frames.sum()) * 768 * 4)
        for x, y in zip(defined(r), want):
            _same(x, y, (precision, "fill 0x%02X" % g.fill))


SEGMENT_CASES = [(T, mode) for T in (1, 2, 37, 513) for mode in ("allspeech", "normal")]


@pytest.mark.parametrize("path,T,mode", [(p, T, m) for p in ("wide", "per_utterance", "frames") for T, m in SEGMENT_CASES]
                         + [("per_utterance", 3941, "long")])
def test_segment(encoders, path, T, mode):
    """sylber_segment on both SYLBER_OPT_SEGMENT paths and sylber_segment_frames (wide path only), with and without features; T = 513
    all-speech takes the wide path's global-slab launch, T = 3941 the per-utterance path's slab kernel (run on that path only)"""
    enc = encoders("bf16", -1 if path == "per_utterance" else 0)
    B = 3
    x = torch.from_numpy(np.stack([syllable_states(T, 500 + T + s, mode=mode) for s in range(B)])).cuda()
    fr = [T, max(1, T - 1), max(1, T // 2)] if path == "frames" else None
    for with_features in (True, False):
        def run(g):
            h = x if g is None else g.guarded_copy(x, "hidden")
            return enc.segment(h, 2.6, 0.8, with_features=with_features, frames=fr)
        plain, guarded = three_runs(run)
        n = plain[1].tolist()
        if mode == "allspeech":
            assert min(n) >= 1
        for g, (seg, nseg, feats) in guarded:
            assert g.covers(seg) and g.covers(nseg) and (feats is None) == (not with_features) and (feats is None or g.covers(feats))
            assert g.handed_out(B * T * 2 * 8) and g.handed_out(B * 4)
            what = (path, T, mode, with_features, "fill 0x%02X" % g.fill)
            _same(nseg, plain[1], what)
            for b in range(B):
                _same(seg[b, :n[b]], plain[0][b, :n[b]], what)
                if with_features:
                    _same(feats[b, :n[b]], plain[2][b, :n[b]], what)
