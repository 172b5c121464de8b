"""Golden vectors for tests/test_oracle_segment.py::test_oracle_vs_reference_seeded_states (survey container only): the
REFERENCE's own ``get_segment`` (sylber/utils/segment_utils.py:72-131) on 40 seeded state sequences of
``syllable_states`` (T = 5 / 77 / 300 frames; modes normal / edge / long), stored in tests/golden/segment_seeded.npz
(inputs by seed, outputs: the segment tables, a float64 checksum of every input).  The oracle must agree bit for bit before
anything is written.  Contains no reference code; never runs on the GPU box.

    python tools/gen_golden_seeded_segment.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import segment_oracle                         # noqa: E402
from sylber_amd.synth_states import syllable_states       # noqa: E402
from tools import ref_shim                                # noqa: E402


def cases():
    """(T, seed, mode) of the 40 cases, in the order the test walks them"""
    return [([5, 77, 300][s % 3], 9000 + s, ["normal", "edge", "long"][s % 3]) for s in range(40)]


def main():
    _, seg_utils, _ = ref_shim.load()
    warnings.simplefilter("ignore")
    Ts, seeds, modes, offs, flat, state_sums = [], [], [], [0], [], []
    for T, seed, mode in cases():
        st = syllable_states(T, seed, mode=mode)
        r = seg_utils.get_segment(st, 2.6, 0.8)
        o = segment_oracle.get_segment(st, 2.6, 0.8)
        assert r.shape == o.shape and np.array_equal(r, o), (T, seed, mode)
        r2 = np.asarray(r).reshape(-1, 2).astype(np.int64)
        Ts.append(T); seeds.append(seed); modes.append(mode)
        flat.append(r2); offs.append(offs[-1] + len(r2))
        state_sums.append(float(st.astype(np.float64).sum()))
    path = os.path.join(ROOT, "tests", "golden", "segment_seeded.npz")
    np.savez_compressed(path, T=np.array(Ts), seed=np.array(seeds), mode=np.array(modes), offsets=np.array(offs),
                        segments=np.concatenate(flat, 0), state_sum=np.array(state_sums))
    print("wrote tests/golden/segment_seeded.npz: %d cases, %d segments" % (len(Ts), offs[-1]))


if __name__ == "__main__":
    main()
