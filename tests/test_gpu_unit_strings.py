"""GPU tier of the unit strings (sylber_amd.align_unit_strings / unit_error_rate, csrc/unit_strings.hip) against
tests/unit_strings_ref.py: ops, costs, cols and subs equal bit for bit -- everything is a small integer, no tolerance is involved.
Shapes are the smallest at which the kernel can go wrong: references around one, two and three strips of 64 rows, hypotheses around
the chunk of 32 anti-diagonal steps and the 128-column ring, empty sides, widths that fill their padded row and widths that do not,
alphabets of 2 (ties everywhere) and 50, one pair of 47 strips, and the longest string on either side."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unit_strings_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu

from sylber_amd import UnitIndex, align_unit_strings, unit_error_rate  # noqa: E402
from sylber_amd import units as units_mod  # noqa: E402

MS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
LS = (0, 1, 31, 32, 33, 64, 65, 96, 129, 300)
CONFIGS = [(1, 2), (2, 3), (3, 3), (8, 50)]               # (W, alphabet): W = 3 is padded to 4 words


def _np(out):
    return tuple(o.cpu().numpy() for o in out)


def _same(a, b):
    assert len(a) == len(b)
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _strings(rng, n, W, A):
    s = rng.integers(0, A, (n, W))
    return s[:, 0] if W == 1 else s


_BATCHES = {}


def _boundary_batch(W, A):
    """every m of MS against every L of LS, with the reference's result, made once"""
    if (W, A) not in _BATCHES:
        rng = np.random.default_rng(1000 * W + A)
        refs, hyps = [], []
        for m in MS:
            for L in LS:
                refs.append(_strings(rng, m, W, A))
                if m and L and (m + L) % 3 == 0:           # a hypothesis cut from the reference: long diagonal runs beside the ties
                    base = np.resize(refs[-1], (L,) + refs[-1].shape[1:])
                    noise = _strings(rng, L, W, A)
                    keep = rng.random(L) < 0.8
                    hyps.append(np.where(keep.reshape((L,) + (1,) * (base.ndim - 1)), base, noise))
                else:
                    hyps.append(_strings(rng, L, W, A))
        _BATCHES[W, A] = (refs, hyps, sref.align_batch(refs, hyps))
    return _BATCHES[W, A]


def _raw(refs, hyps, W, pairing=1, fill=None):
    """``sylber_unit_strings_align`` itself, all pairs in one launch, with the walk's own counts -> (cols, subs, ops, costs, ops_walk)
    as int32 arrays"""
    import ctypes
    from sylber_amd import _lib
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
    i32p = ctypes.POINTER(ctypes.c_int32)

    def flat(strings):
        off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int32)
        rows = np.concatenate([np.asarray(s, np.int64).reshape(len(s), W) for s in strings] + [np.zeros((1, W), np.int64)])
        return torch.from_numpy(rows.astype(np.int32)).to(dev), off

    rd, ro = flat(refs)
    hd, ho = flat(hyps)
    S, total = len(refs), int(ro[-1])
    cols, subs = (torch.full((total + 1,), 7, dtype=torch.int32, device=dev) for _ in range(2))
    ops, walk = (torch.full((S, 4), 7, dtype=torch.int32, device=dev) for _ in range(2))
    cost = torch.full((S,), 7, dtype=torch.int32, device=dev)
    size = int(lib.sylber_unit_strings_workspace_bytes(ro.ctypes.data_as(i32p), ho.ctypes.data_as(i32p), S, pairing))
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    with torch.cuda.device(dev):
        _lib.check(lib.sylber_unit_strings_align(_vp(rd), ro.ctypes.data_as(i32p), _vp(hd), ho.ctypes.data_as(i32p), W, S, pairing,
                                                 _vp(cols), _vp(subs), _vp(ops), _vp(cost), _vp(walk), _vp(ws), _stream(dev)),
                   "sylber_unit_strings_align")
    out = tuple(t.cpu().numpy() for t in (cols, subs, ops, cost, walk))
    assert out[0][total] == 7 and out[1][total] == 7       # nothing past the last reference unit
    return (out[0][:total], out[1][:total]) + out[2:]


def _identities(cols, subs, ops, costs, off, hyps, W):
    m, L = np.diff(off), np.array([len(h) for h in hyps])
    assert np.array_equal(ops[:, :3].sum(1), m) and np.array_equal(ops[:, [0, 1, 3]].sum(1), L)
    sums = np.array([subs[a:b].sum() for a, b in zip(off[:-1], off[1:])])
    assert np.array_equal(costs, sums + W * ops[:, 3])
    assert np.array_equal(np.array([(cols[a:b] < 0).sum() for a, b in zip(off[:-1], off[1:])]), ops[:, 2])


# ---- one call with every boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, A", CONFIGS)
def test_one_call_with_every_boundary(W, A):
    refs, hyps, want = _boundary_batch(W, A)
    ops, costs = _np(align_unit_strings(refs, hyps))
    assert _same((ops, costs), want[2:4])
    got = _np(align_unit_strings(refs, hyps, pairing=True))
    assert got[0].dtype == np.int64 and _same(got, want)
    _identities(*got, hyps, W)
    raw = _raw(refs, hyps, W)
    assert all(np.array_equal(x, y) for x, y in zip(raw[:4], want[:4]))
    assert np.array_equal(raw[4], raw[2])                  # the walk over the codes counts what the cells carried
    raw0 = _raw(refs, hyps, W, pairing=0)
    assert np.array_equal(raw0[2], want[2]) and np.array_equal(raw0[3], want[3])
    assert (raw0[0] == 7).all() and (raw0[1] == 7).all() and (raw0[4] == 7).all()       # counts only: nothing else is written


@pytest.mark.parametrize("W, A", CONFIGS)
def test_against_the_existing_kernel(W, A):
    """for 1 <= m <= 64 and L >= 1: ``UnitIndex(h).align_phrases([r], [[[0, L]]], free_start=False)``, cols as positions"""
    refs, hyps, _ = _boundary_batch(W, A)
    pick = [s for s in range(len(refs)) if 1 <= len(refs[s]) <= 64 and len(hyps[s]) >= 1]
    assert len(pick) == 3 * 9
    cols, subs, ops, costs, off = _np(align_unit_strings([refs[s] for s in pick], [hyps[s] for s in pick], pairing=True))
    for e, s in enumerate(pick):
        L = len(hyps[s])
        c, sb, o, cost = _np(UnitIndex(hyps[s]).align_phrases([refs[s]], torch.tensor([[[0, L]]]), free_start=False))
        assert np.array_equal(c[0, 0], cols[off[e]:off[e + 1]]) and np.array_equal(sb[0, 0], subs[off[e]:off[e + 1]])
        assert np.array_equal(o[0, 0], ops[e]) and cost[0, 0] == costs[e]
        assert c.dtype == cols.dtype and sb.dtype == subs.dtype and o.dtype == ops.dtype and cost.dtype == costs.dtype


def test_inputs_on_the_device_and_in_either_form():
    refs, hyps, want = _boundary_batch(1, 2)
    dev = [torch.from_numpy(np.asarray(r)).cuda() for r in refs]
    wide = [np.asarray(h).reshape(-1, 1).astype(np.int32) for h in hyps]
    assert _same(_np(align_unit_strings(dev, wide, pairing=True)), want)
    mixed = [d if i % 2 else r for i, (d, r) in enumerate(zip(dev, refs))]
    assert _same(_np(align_unit_strings(mixed, [{"units": h} for h in hyps])), want[2:4])
    assert _same(_np(align_unit_strings(tuple(refs), tuple(hyps), device="cuda:0")), want[2:4])


# ---- long strings -------------------------------------------------------------------------------------------------------------------
def test_one_pair_of_47_strips():
    rng = np.random.default_rng(5)
    r, h = rng.integers(0, 2, 3000), rng.integers(0, 2, 2900)      # two symbols: ties everywhere
    want = sref.align_batch([r], [h])
    assert _same(_np(align_unit_strings([r], [h])), want[2:4])
    got = _np(align_unit_strings([r], [h], pairing=True))
    assert _same(got, want)
    _identities(*got, [h], 1)
    raw = _raw([r], [h], 1)
    assert np.array_equal(raw[4], want[2]) and np.array_equal(raw[0], want[0])


@pytest.mark.parametrize("m, L", [(65536, 70), (70, 65536)])
def test_the_longest_string_on_either_side(m, L):
    rng = np.random.default_rng(m % 7)
    r, h = rng.integers(0, 3, (m, 2)), rng.integers(0, 3, (L, 2))
    want = sref.align_batch([r], [h])
    assert _same(_np(align_unit_strings([r], [h])), want[2:4])


# ---- independence -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """40 pairs over two symbols, from empty to four strips, with their reference result"""
    rng = np.random.default_rng(6)
    ms = rng.integers(0, 260, 40)
    Ls = rng.integers(0, 200, 40)
    ms[3], Ls[5], ms[8], Ls[8] = 0, 0, 0, 0
    refs = [rng.integers(0, 2, (int(m), 2)) for m in ms]
    hyps = [rng.integers(0, 2, (int(L), 2)) for L in Ls]
    return refs, hyps, sref.align_batch(refs, hyps)


def _split(out, off):
    """a pairing result per pair"""
    return [(out[0][a:b], out[1][a:b], out[2][s], out[3][s]) for s, (a, b) in enumerate(zip(off[:-1], off[1:]))]


def test_nothing_depends_on_chunks_order_company_or_the_workspace(mixed, monkeypatch):
    refs, hyps, want = mixed
    S = len(refs)
    for pairing in (False, True):
        ref = want if pairing else want[2:4]
        assert _same(_np(align_unit_strings(refs, hyps, pairing=pairing)), ref)
        for kw in (dict(pair_chunk=1), dict(pair_chunk=7), dict(_workspace_fill=0x00), dict(_workspace_fill=0xFF),
                   dict(pair_chunk=7, _workspace_fill=0xFF), dict(pair_chunk=1000)):
            assert _same(_np(align_unit_strings(refs, hyps, pairing=pairing, **kw)), ref), kw
        # launches cut by the workspace bound, not by pair_chunk
        need = units_mod.unit_strings_workspace_bytes([len(r) for r in refs], [len(h) for h in hyps], pairing)
        with monkeypatch.context() as mp:
            mp.setattr(units_mod, "ALIGN_WORKSPACE_BYTES", int(need.max()) + 48 + 256 + 4096)
            assert _same(_np(align_unit_strings(refs, hyps, pairing=pairing, _workspace_fill=0xFF)), ref)
        perm = np.random.default_rng(8).permutation(S)
        got = _np(align_unit_strings([refs[s] for s in perm], [hyps[s] for s in perm], pairing=pairing))
        if pairing:
            back = dict(zip(perm.tolist(), _split(got, got[4])))
            assert all(_same(back[s], one) for s, one in enumerate(_split(want, want[4])))
        else:
            assert np.array_equal(got[0], want[2][perm]) and np.array_equal(got[1], want[3][perm])
        for s in range(S):                                 # each pair alone
            got = _np(align_unit_strings([refs[s]], [hyps[s]], pairing=pairing))
            if pairing:
                assert _same(_split(got, got[4])[0], _split(want, want[4])[s]), s
            else:
                assert np.array_equal(got[0][0], want[2][s]) and got[1][0] == want[3][s], s
    for fill in (0x00, 0xFF):
        raw = _raw(refs, hyps, 2, fill=fill)
        assert all(np.array_equal(x, y) for x, y in zip(raw[:4], want[:4])) and np.array_equal(raw[4], raw[2])


def test_no_pairs_no_launch():
    ops, costs = align_unit_strings([], [])
    assert ops.shape == (0, 4) and costs.shape == (0,) and ops.dtype == costs.dtype == torch.int32 and ops.is_cuda
    cols, subs, ops, costs, off = align_unit_strings([], [], pairing=True)
    assert cols.shape == subs.shape == (0,) and cols.dtype == torch.int64 and subs.dtype == torch.int32 and off.tolist() == [0]
    cols, subs, ops, costs, off = _np(align_unit_strings([np.zeros(0, np.int64)] * 2, [np.zeros(0, np.int64)] * 2, pairing=True))
    assert cols.shape == (0,) and not ops.any() and not costs.any() and off.tolist() == [0, 0, 0]


# ---- unit_error_rate ----------------------------------------------------------------------------------------------------------------
def test_unit_error_rate_totals(mixed):
    refs, hyps, want = mixed
    res = unit_error_rate(refs, hyps)
    tot = want[2].astype(np.int64).sum(0)
    assert [res.equal, res.substituted, res.deleted, res.inserted] == tot.tolist()
    assert res.ref_units == sum(len(r) for r in refs) == tot[:3].sum() and res.hyp_units == sum(len(h) for h in hyps)
    assert res.uer == tot[1:].sum() / res.ref_units and res.weighted == want[3].astype(np.int64).sum() / (2 * res.ref_units)
    assert _same(_np((res.ops, res.costs)), want[2:4])
    assert _same(_np((unit_error_rate(refs, hyps, pair_chunk=3).ops,)), want[2:3])
    same = unit_error_rate(refs, refs)
    assert same.uer == 0 and same.weighted == 0 and same.equal == same.ref_units == same.hyp_units
    assert "uer=" in repr(res)
    with pytest.raises(ValueError, match="at least one reference unit"):
        unit_error_rate([np.zeros(0, np.int64)], [np.array([1, 2])])
    with pytest.raises(ValueError, match="at least one reference unit"):
        unit_error_rate([], [])


def test_unit_error_rate_of_two_precisions():
    """two 2 s clips tokenised in bf16 and in fp32: the call runs on what ``tokenize`` returns, and counts what the reference counts
    on the same ids"""
    from sylber_amd import KMQuantizer, SegmentSynthesis
    from sylber_amd.synth import syllable_wave
    from sylber_amd.weights import synthetic_mlp_state_dict, synthetic_regressor_state_dict, synthetic_state_dict
    sd = {"speech_model." + k: v for k, v in synthetic_state_dict(0, num_layers=9).items()}
    sd.update({"input_model." + k: v for k, v in synthetic_mlp_state_dict(1).items()})
    sd.update({"regressor." + k: v for k, v in synthetic_regressor_state_dict(0).items()})
    g = torch.Generator().manual_seed(23)
    c1 = torch.randn(64, 768, generator=g) * 0.09          # at the scale of the synthetic encoder's hidden states
    x = torch.stack([syllable_wave(32000, 21)[0], syllable_wave(32000, 22)[0]]).cuda()
    mask = torch.ones_like(x)
    toks, thr = {}, None
    for prec in ("fp32", "bf16"):
        syn = SegmentSynthesis(model_ckpt=sd, device="cuda:0", precision=prec, quantizer=KMQuantizer(c1, device="cuda:0"))
        if thr is None:                                    # a threshold inside the range of the synthetic encoder's norms
            hidden = syn.speech_model.forward(x.contiguous(), [32000, 32000])
            frames = syn.speech_model.frame_counts([32000, 32000])
            norms = torch.cat([torch.sqrt((hidden[b, :f].double() ** 2).sum(-1) + 1e-8) for b, f in enumerate(frames)])
            thr = float(np.round(torch.quantile(norms, 0.4).item(), 2))
        toks[prec] = syn.tokenize(x, attention_mask=mask, normthreshold=thr)
        assert len(toks[prec]) == 2 and all(len(t["units"]) > 0 for t in toks[prec])
    res = unit_error_rate(toks["fp32"], toks["bf16"])
    want = sref.align_batch([t["units"] for t in toks["fp32"]], [t["units"] for t in toks["bf16"]])
    print("fp32 against bf16: %r" % (res,))
    assert _same(_np((res.ops, res.costs)), want[2:4])
    assert res.ref_units == sum(len(t["units"]) for t in toks["fp32"]) and res.hyp_units == sum(len(t["units"]) for t in toks["bf16"])
    assert 0 <= res.uer and unit_error_rate(toks["bf16"], toks["bf16"]).uer == 0
    assert _same(_np(align_unit_strings(toks["fp32"], toks["bf16"], pairing=True)), want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    one = [np.array([1, 2, 3])]
    with pytest.raises(ValueError, match="equally long, got 1 and 2"):
        align_unit_strings(one, one * 2)
    with pytest.raises(ValueError, match="refs have W = 1, hyps have W = 2"):
        align_unit_strings(one, [np.zeros((2, 2), np.int64)])
    with pytest.raises(ValueError, match="expected W = 2, got 3"):
        align_unit_strings([np.zeros((2, 2), np.int64), np.zeros((2, 3), np.int64)], one * 2)
    for W in (0, 9):
        with pytest.raises(ValueError, match=r"the width W must be in \[1, 8\], got %d" % W):
            align_unit_strings([np.zeros((2, W), np.int64)], one)
    for bad in (np.array([0.5, 1.0]), np.array([True, False]), torch.tensor([1.0], device="cuda"), torch.tensor([1.5])):
        with pytest.raises(ValueError, match="must be integers"):
            align_unit_strings(one, [bad])
    for bad in (np.array([1, -1]), torch.tensor([3, -2], device="cuda"), np.array([2 ** 31]), np.array([2 ** 31], np.uint64)):
        with pytest.raises(ValueError, match=r"unit ids lie in \[0, 2\*\*31 - 1\]"):
            align_unit_strings([bad], one)
    assert _np(align_unit_strings([np.array([2 ** 31 - 1, 0])], [np.array([2 ** 31 - 1], np.uint64)]))[0].tolist() == [[1, 0, 1, 0]]
    with pytest.raises(ValueError, match="hyps\\[0\\] has 65537 units, more than 65536"):
        align_unit_strings(one, [np.zeros(65537, np.int64)])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="pair_chunk must be an integer >= 1"):
            align_unit_strings(one, one, pair_chunk=bad)
    with pytest.raises(ValueError, match="sequence of unit strings"):
        align_unit_strings(np.arange(3), one)


def test_an_oversized_pairing_pair_is_refused_before_anything_is_allocated():
    r = np.zeros(40000, np.int64)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(ValueError, match=r"pair 1 \(40000 x 40000 units\).*pairing=False"):
        align_unit_strings([np.array([1]), r], [np.array([1]), r], pairing=True)
    assert torch.cuda.max_memory_allocated() == before
    ops, costs = _np(align_unit_strings([r[:100]], [r[:100]], pairing=False))      # the mode the message names takes such pairs
    assert ops.tolist() == [[100, 0, 0, 0]] and costs.tolist() == [0]
