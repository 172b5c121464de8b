"""CPU tier, packed batches: the slot layout (sylber_packed_layout) against a Python restatement, and the host staging helper.

A packed batch gives clip b a slot of frames at offset offsets[b]: every conv layer's valid rows of a call of the clip's own length
(the same bound sylber_padded_frames rounds up to 32), rounded up to whole 64-key attention tiles."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CK = [10, 3, 3, 3, 3, 2, 2]
CS = [5, 2, 2, 2, 2, 2, 2]


def ref_frames_and_need(n):
    """frames of an n-sample clip and the rows per frame its conv layers need: max_i ceil(L_i / 2^(6 - i))"""
    need = 0
    for i in range(7):
        n = (n - CK[i]) // CS[i] + 1
        f = 1 << (6 - i)
        need = max(need, -(-n // f))
    return n, need


def ref_layout(lengths):
    off, fr = [0], []
    for n in lengths:
        t, need = ref_frames_and_need(n)
        fr.append(t)
        off.append(off[-1] + -(-need // 64) * 64)
    return np.array(off, np.int32), np.array(fr, np.int32)


def samples_for_frames(t):
    """the shortest clip with t frames"""
    return 400 + 320 * (t - 1)


def test_layout_matches_restatement():
    from sylber_amd import _lib
    from sylber_amd.segmenter import packed_layout
    lib = _lib.load()
    rng = np.random.default_rng(7)
    lengths = [400, 401, 719, 720, samples_for_frames(64), samples_for_frames(65), samples_for_frames(64) - 1,
               samples_for_frames(65536), samples_for_frames(65537), 160000, 960000]
    lengths += [int(x) for x in rng.integers(400, 20 * 16000, 64)]
    off, fr = packed_layout(lengths)
    roff, rfr = ref_layout(lengths)
    assert np.array_equal(off, roff) and np.array_equal(fr, rfr)
    assert off[0] == 0 and (np.diff(off) % 64 == 0).all()
    for b, n in enumerate(lengths):
        assert fr[b] == lib.sylber_num_frames(n)
        assert off[b + 1] - off[b] >= fr[b]
        assert off[b + 1] - off[b] >= lib.sylber_padded_frames(n) - 31      # every conv layer's valid rows fit the slot
    assert fr[0] == 1 and off[1] == 64                                       # 400 samples: one frame, one tile
    i64 = lengths.index(samples_for_frames(65536))
    assert fr[i64] == 65536 and fr[i64 + 1] == 65537
    assert off[i64 + 1] - off[i64] == 65536 + 64                             # the conv rows need one frame more than T here
    assert off[i64 + 2] - off[i64 + 1] == 65536 + 64


def test_layout_slot_covers_conv_rows_at_multiples_of_64():
    """T_b % 64 == 0 is where round_up(T_b, 64) alone would be one frame short of the conv layers' rows"""
    from sylber_amd.segmenter import packed_layout
    short = []
    for t in range(1, 2000):
        for n in (samples_for_frames(t), samples_for_frames(t + 1) - 1):
            ft, need = ref_frames_and_need(n)
            assert ft == t
            if need > -(-t // 64) * 64:
                short.append(n)
    assert short                                                             # such lengths exist
    off, fr = packed_layout(short)
    for b, n in enumerate(short):
        assert off[b + 1] - off[b] >= ref_frames_and_need(n)[1]


def test_layout_rejects_short_clips_and_overflow():
    from sylber_amd import _lib
    from sylber_amd.segmenter import packed_layout
    with pytest.raises(ValueError):
        packed_layout([16000, 399])
    with pytest.raises(ValueError):
        packed_layout([])
    with pytest.raises(ValueError, match="too long"):
        packed_layout([2 ** 31 - 1] * 2)                                    # 2 x 6.7 M frames x 320 samples > 2^31
    lib = _lib.load()
    off, fr = (_lib.ctypes.c_int32 * 3)(), (_lib.ctypes.c_int32 * 2)()
    assert lib.sylber_packed_layout((_lib.ctypes.c_int32 * 2)(16000, 300), 2, off, fr) == 1
    assert b"400" in lib.sylber_last_error()
    # the largest batch that fits: offsets[B] x 320 <= 2^31 - 1
    n = samples_for_frames(3_000_000)
    o, _ = packed_layout([n, n])
    assert 320 * int(o[-1]) <= 2 ** 31 - 1


def test_stage_packed_places_clips_at_slots():
    from sylber_amd.segmenter import SLOT_SAMPLES, _stage_packed, packed_layout
    rng = np.random.default_rng(3)
    lengths = [400, 16000, 5000, samples_for_frames(128)]
    rows = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in lengths]
    rows[2] = rows[2].to(torch.float64)                                      # converted on the way
    off, _ = packed_layout(lengths)
    stage = np.full(SLOT_SAMPLES * int(off[-1]), np.nan, np.float32)
    _stage_packed(stage, rows, lengths, off, 0, 2)
    _stage_packed(stage, rows, lengths, off, 2, 4)
    for b, n in enumerate(lengths):
        a, e = SLOT_SAMPLES * int(off[b]), SLOT_SAMPLES * int(off[b + 1])
        assert np.array_equal(stage[a:a + n], rows[b].to(torch.float32).numpy())
        assert (stage[a + n:e] == 0).all() and not np.signbit(stage[a + n:e]).any()
    assert not np.isnan(stage).any()


def test_header_and_exports_declare_the_packed_entry_points():
    from sylber_amd import _lib
    with open(os.path.join(ROOT, "include", "sylber_hip.h")) as f:
        hdr = f.read()
    for name in ("sylber_packed_layout", "sylber_forward_packed", "sylber_segment_packed", "sylber_packed_gather"):
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        assert hasattr(_lib.load(), name)
