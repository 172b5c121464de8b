"""CPU tier, packed decoder batches: the decoder's slot layout (sylber_cfm_packed_layout) against a Python restatement.

Clip b of a packed decoder batch gets round_up(16 + T_b, 64) rows: its 16 register rows, its T_b frame rows and zero rows to the slot
end.  The packed attention loads 64-key tiles from the slot start, so a slot that is not a whole number of tiles would let a clip's last
tile reach into its neighbour."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_slots(frames):
    off = [0]
    for t in frames:
        off.append(off[-1] + -(-(16 + t) // 64) * 64)
    return np.array(off, np.int32)


def test_layout_matches_restatement():
    from sylber_amd.synthesis import cfm_packed_layout
    rng = np.random.default_rng(11)
    frames = [1, 47, 48, 49, 111, 112, 113, 500, 999, 1000] + [int(x) for x in rng.integers(1, 3000, 64)]
    off = cfm_packed_layout(frames)
    assert off.dtype == np.int32 and off.shape == (len(frames) + 1,)
    assert np.array_equal(off, ref_slots(frames))
    assert off[0] == 0 and (np.diff(off) % 64 == 0).all()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.diff(off))]))           # slots follow each other
    for b, t in enumerate(frames):
        assert 16 + t <= off[b + 1] - off[b] < 16 + t + 64


def test_layout_edges():
    """16 + T_b = 64 and 128 fill their slots exactly; one frame more opens a new tile"""
    from sylber_amd.synthesis import cfm_packed_layout
    off = cfm_packed_layout([48, 112, 1, 49, 113])
    assert list(np.diff(off)) == [64, 128, 64, 128, 192]
    assert list(off) == [0, 64, 192, 256, 384, 576]


def test_layout_single_clip():
    from sylber_amd.synthesis import cfm_packed_layout
    assert list(cfm_packed_layout([1])) == [0, 64]
    assert list(cfm_packed_layout([496])) == [0, 512]


def test_layout_refuses_bad_counts():
    from sylber_amd import _lib
    from sylber_amd.synthesis import cfm_packed_layout
    for bad in ([], [0], [5, -1], [2 ** 24]):
        with pytest.raises(ValueError):
            cfm_packed_layout(bad)
    lib = _lib.load()
    c = _lib.ctypes.c_int32
    off = (c * 3)()
    assert lib.sylber_cfm_packed_layout((c * 2)(16, 0), 2, off) == 1
    assert b"sylber_cfm_packed_layout" in lib.sylber_last_error()
    assert lib.sylber_cfm_packed_layout((c * 1)(16), 0, off) == 1
    assert lib.sylber_cfm_packed_layout((c * 2)(2 ** 23, 2 ** 23), 2, off) == 1           # 2^24 rows and more do not fit
    assert lib.sylber_cfm_packed_layout((c * 2)(100, 30), 2, off) == 0
    assert list(off) == [0, 128, 192]


def test_packed_entry_points_refuse_before_touching_a_device():
    """the argument checks run on the host: a null handle or bad counts fail with a message naming the call"""
    from sylber_amd import _lib
    lib = _lib.load()
    c = _lib.ctypes.c_int32
    assert lib.sylber_cfm_workspace_bytes_packed(None, (c * 1)(5), 1) == -1
    assert b"sylber_cfm_workspace_bytes_packed" in lib.sylber_last_error()
    assert lib.sylber_cfm_sample_packed(None, None, (c * 1)(5), 1, 5, None, 1.0, None, None, None) == 1
    assert b"sylber_cfm_sample_packed" in lib.sylber_last_error()
    assert lib.sylber_condition_packed(None, None, None, None, 1, None, None, None, 1, 1, 1.0, None, None, None, None) == 1
    assert b"sylber_condition_packed" in lib.sylber_last_error()
    assert lib.sylber_condition_units_packed(None, None, 1, None, 0, None, None, None, None, 1, 1, None, None, None) == 1
    assert b"sylber_condition_units_packed" in lib.sylber_last_error()


def test_header_and_exports_declare_the_packed_decoder():
    from sylber_amd import _lib
    with open(os.path.join(ROOT, "include", "sylber_hip.h")) as f:
        hdr = f.read()
    for name in ("sylber_cfm_packed_layout", "sylber_cfm_workspace_bytes_packed", "sylber_cfm_sample_packed",
                 "sylber_condition_packed_workspace_floats", "sylber_condition_packed", "sylber_condition_units_packed"):
        assert name + "(" in hdr, name
        assert name in _lib.EXPORTS, name
        assert hasattr(_lib.load(), name)
