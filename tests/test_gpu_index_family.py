"""GPU tier, the host rules that ``SyllableIndex``, ``IVFSyllableIndex``, ``PQSyllableIndex`` and ``IVFPQSyllableIndex`` share
(sylber_amd/_index.py), pinned across the four classes:

* the saved file: its keys, dtypes and shapes, the per-row arrays in id order, before and after ``drop_rows``, and the refusal of
  another class's file;
* ``provenance``: the same answer from every class, with the rows held and dropped, and after a save / load round trip.

One small data set: 300 rows of 32 columns from two ``add`` calls (200 rows with integer-span provenance, 100 without), one row with a
NaN (in no list, masked), 3 given centroids and 2 x 256 given codebook centroids; nothing is trained."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N1, N2, D, M, NLIST = 200, 100, 32, 2, 3
N = N1 + N2
CLIPS = 4                       # the first add: 4 clips of 50 segments
NAN_ROW = 7
KINDS = ["flat", "ivf", "pq", "ivfpq"]
BASE_KEYS = {"metric", "features", "groups", "provenance", "span_int"}
PQ_KEYS = {"metric", "codebooks", "codes", "bad", "groups", "provenance", "span_int", "rows_held", "features"}
KEYS = {"flat": BASE_KEYS, "ivf": BASE_KEYS | {"centroids", "labels"}, "pq": PQ_KEYS, "ivfpq": PQ_KEYS | {"centroids", "labels"}}
IDS = [-1, N, 57, N1 + 50, NAN_ROW]


class Data:
    def __init__(self):
        rng = np.random.default_rng(20240607)
        self.x = rng.standard_normal((N, D)).astype(np.float32)
        self.x[NAN_ROW, 3] = np.nan
        self.centroids = rng.standard_normal((NLIST, D)).astype(np.float32)
        self.codebooks = rng.standard_normal((M, 256, D // M)).astype(np.float32)
        per = N1 // CLIPS
        starts = rng.integers(0, 1000, (CLIPS, per)).astype(np.int64)
        self.outs = [{"segment_features": self.x[c * per:(c + 1) * per], "segments": np.stack([starts[c], starts[c] + 1 + c], 1)}
                     for c in range(CLIPS)]
        self.g2 = rng.integers(100, 105, N2).astype(np.int32)
        self.groups = np.concatenate([np.repeat(np.arange(CLIPS, dtype=np.int32), per), self.g2])
        self.bad = np.zeros(N, np.uint8)
        self.bad[NAN_ROW] = 1

        def prov(i):
            c, s = divmod(i, per)
            return (c, s, int(starts[c, s]), int(starts[c, s]) + 1 + c)
        self.provenance = [None, None, prov(57), None, prov(NAN_ROW)]

    def make(self, kind):
        """an index of this kind over the first add, then the second add through the class itself"""
        from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex, SyllableIndex
        ix = SyllableIndex.from_outputs(self.outs, device=DEV)
        if kind == "ivf":
            ix = IVFSyllableIndex.build(ix, centroids=self.centroids)
        elif kind == "pq":
            ix = PQSyllableIndex.build(ix, M, codebooks=self.codebooks)
        elif kind == "ivfpq":
            ix = IVFPQSyllableIndex.build(ix, M=M, centroids=self.centroids, codebooks=self.codebooks)
        assert list(ix.add(self.x[N1:], groups=self.g2)) == list(range(N1, N))
        return ix


@pytest.fixture(scope="module")
def data():
    return Data()


def _cls(kind):
    import sylber_amd
    return {"flat": sylber_amd.SyllableIndex, "ivf": sylber_amd.IVFSyllableIndex, "pq": sylber_amd.PQSyllableIndex,
            "ivfpq": sylber_amd.IVFPQSyllableIndex}[kind]


def _states(kind):
    return [False, True] if kind in ("pq", "ivfpq") else [False]


def _check_file(path, kind, ix, data, dropped):
    z = np.load(path, allow_pickle=False)
    assert set(z.files) == KEYS[kind] and len(z.files) == len(KEYS[kind])
    assert str(z["metric"]) == "l2" and bool(z["span_int"])
    f = z["features"]
    assert f.dtype == np.float32 and f.shape == ((0, D) if dropped else (N, D))
    if not dropped:
        assert np.array_equal(f, data.x, equal_nan=True)
    assert z["groups"].dtype == np.int32 and np.array_equal(z["groups"], data.groups)
    assert z["provenance"].dtype == np.float64 and z["provenance"].shape == (N, 4)
    if kind in ("ivf", "ivfpq"):
        assert z["centroids"].dtype == np.float32 and np.array_equal(z["centroids"], data.centroids)
        assert z["labels"].dtype == np.int32 and np.array_equal(z["labels"], ix.labels.cpu().numpy())
        assert z["labels"][NAN_ROW] == -1 and (np.delete(z["labels"], NAN_ROW) >= 0).all()
    if kind in ("pq", "ivfpq"):
        assert z["codebooks"].dtype == np.float32 and np.array_equal(z["codebooks"], data.codebooks)
        assert z["codes"].dtype == np.uint8 and z["codes"].shape == (N, M) and np.array_equal(z["codes"], ix.codes.cpu().numpy())
        assert z["bad"].dtype == np.uint8 and np.array_equal(z["bad"], data.bad)
        assert bool(z["rows_held"]) == (not dropped)


@pytest.mark.parametrize("kind", KINDS)
def test_saved_file_format(kind, data, tmp_path):
    ix = data.make(kind)
    for dropped in _states(kind):
        if dropped:
            ix.drop_rows()
        path = str(tmp_path / ("%s_%d.npz" % (kind, dropped)))
        ix.save(path)
        _check_file(path, kind, ix, data, dropped)
    if kind == "ivfpq":                                     # the per-row arrays are in id order, not in the index's list order
        assert np.array_equal(ix.codes.cpu().numpy()[ix._rid.cpu().numpy()], ix._codes.cpu().numpy())
        assert not np.array_equal(ix._rg.cpu().numpy(), data.groups)


def test_load_refuses_another_class_file(data, tmp_path):
    paths = {}
    for kind in ("flat", "ivf", "pq"):
        paths[kind] = str(tmp_path / (kind + ".npz"))
        data.make(kind).save(paths[kind])
    for kind, other in (("ivf", "flat"), ("pq", "ivf"), ("ivfpq", "pq")):
        with pytest.raises(ValueError):
            _cls(kind).load(paths[other], device=DEV)


def _check_provenance(ix, data):
    for ids in (IDS, np.array(IDS), torch.tensor(IDS, device=DEV)):
        got = ix.provenance(ids)
        assert got == data.provenance
        for p in got:
            assert p is None or all(type(v) is int for v in p)


@pytest.mark.parametrize("kind", KINDS)
def test_provenance_is_one_answer(kind, data, tmp_path):
    ix = data.make(kind)
    assert len(ix) == N
    for dropped in _states(kind):
        if dropped:
            ix.drop_rows()
        _check_provenance(ix, data)
        path = str(tmp_path / ("%s_%d.npz" % (kind, dropped)))
        ix.save(path)
        back = _cls(kind).load(path, device=DEV)
        assert len(back) == N
        _check_provenance(back, data)
