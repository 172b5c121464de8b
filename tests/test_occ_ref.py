"""CPU tier: the properties that "Every occurrence of a phrase" (include/sylber_hip.h, tests/occ_ref.py) rests on, checked with the
project's own fp32 recurrence on random, small-integer (exact ties) and +inf-holed cost matrices, m 1..8, L 1..40; and the new
entries in the library's interface."""
import numpy as np

import dtw_ref
import occ_ref as O

INF = np.float32(np.inf)


def _matrices(n=3000, seed=0):
    rng = np.random.default_rng(seed)
    for i in range(n):
        m, L = int(rng.integers(1, 9)), int(rng.integers(1, 41))
        kind = i % 3
        if kind == 0:
            d = rng.random((m, L)).astype(np.float32)
        elif kind == 1:
            d = rng.integers(0, 3, (m, L)).astype(np.float32)            # exact ties in every sum
        else:
            d = rng.integers(0, 4, (m, L)).astype(np.float32)
            d[rng.random((m, L)) < 0.25] = INF                            # holes, whole +inf columns and rows among them
            if i % 2:
                d[rng.integers(0, m)] = np.where(rng.random(L) < 0.7, INF, d[0])
        yield d


MATS = list(_matrices())
ROWS = [O.last_row(d) for d in MATS]


def test_the_wavefront_form_is_the_loop():
    for d, (E, st) in zip(MATS[:600], ROWS):
        E2, st2 = O.last_row_loop(d)
        assert np.array_equal(E.view(np.uint32), E2.view(np.uint32))
        fin = E < INF
        assert np.array_equal(st[fin], st2[fin])
        assert np.array_equal(E2.view(np.uint32), dtw_ref.dtw_loop(d)[3][-1].view(np.uint32))


def test_starts_of_finite_columns_do_not_decrease_and_no_family_is_split():
    for E, st in ROWS:
        fin = np.nonzero(E < INF)[0]
        assert (np.diff(st[fin]) >= 0).all()
        assert (st[fin] <= fin).all()
        fams = O.families(E, st)
        starts = [f[1] for f in fams]
        assert len(set(starts)) == len(starts) == len(set(st[fin].tolist()))        # grouping neighbours split no family
        assert starts == sorted(starts) and [f[2] for f in fams] == sorted(f[2] for f in fams)
        for c, a, e in fams:
            mine = fin[st[fin] == a]
            assert c == E[mine].min() and e == mine[E[mine] == c][0] and a <= e


def test_emitted_spans_are_pairwise_disjoint_real_paths():
    n = 0
    for E, st in ROWS:
        occ = O.one_pass(O.families(E, st))
        assert bool(occ) == bool((E < INF).any())
        for (c0, a0, e0), (c1, a1, e1) in zip(occ, occ[1:]):
            assert a0 <= e0 < a1 <= e1
        for c, a, e in occ:
            assert E[e] == c and st[e] == a and c < INF
        n += len(occ)
    assert n > 2 * len(ROWS)                                             # the matrices do hold several occurrences


def test_the_one_state_form_of_the_kernels_is_the_family_pass():
    for E, st in ROWS:
        assert O.one_pass_columns(E, st) == O.one_pass(O.families(E, st))


def test_consequence_a_the_best_occurrence_is_search_phrases():
    for d, (E, st) in zip(MATS, ROWS):
        occ = O.one_pass(O.families(E, st))
        cost, start, end, _ = dtw_ref.dtw_loop(d)
        if not cost < INF:
            assert not occ
            continue
        c, a, e = min(occ, key=lambda f: (f[0], f[1]))
        assert np.float32(c).view(np.uint32) == np.float32(cost).view(np.uint32) and (a, e) == (start, end)


def test_one_row_phrases_every_finite_column_is_an_occurrence():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 3, (1, 30)).astype(np.float32)
    d[0, [3, 4, 17]] = INF
    d[0, 20] = np.nan                                                    # NaN counts as +inf
    occ = O.occurrences(d)
    fin = [j for j in range(30) if j not in (3, 4, 17, 20)]
    assert occ == [(d[0, j], j, j) for j in fin]


def test_one_pass_is_not_greedy_suppression():
    # families A = (4, columns 0..1), B = (2, 1..2), C = (1, 2..3): A and C are disjoint, both share a column with B, A > B > C
    d = np.array([[1, 1, 1, 3],
                  [4, 3, 1, 0]], np.float32)
    fams = O.families(*O.last_row(d))
    assert fams == [(4.0, 0, 1), (2.0, 1, 2), (1.0, 2, 3)]
    assert O.one_pass(fams) == [(1.0, 2, 3)]                             # B beats A, C beats B: only C
    assert O.greedy(fams) == [(4.0, 0, 1), (1.0, 2, 3)]                  # suppression by cost would keep A beside C
    differ = sum(O.one_pass(f) != O.greedy(f) for f in (O.families(E, st) for E, st in ROWS))
    assert 0 < differ < len(ROWS) // 4                                   # the two rules are different rules, not rarely


def test_rank_orders_by_cost_then_first_row_and_pads():
    offsets = np.array([0, 4, 10])
    occ = [[(np.float32(2), 0, 1), (np.float32(1), 3, 3)], [(np.float32(1), 0, 2), (np.float32(2), 4, 5)]]
    c, s, sp = O.rank(occ, offsets, 5)
    assert c.tolist() == [1, 1, 2, 2, np.inf] and s.tolist() == [0, 1, 0, 1, -1]
    assert sp.tolist() == [[3, 4], [4, 7], [0, 2], [8, 10], [-1, -1]]
    c, s, sp = O.rank(occ, offsets, 2, admissible=[False, True])
    assert s.tolist() == [1, 1] and sp.tolist() == [[4, 7], [8, 10]]


def test_the_entries_are_declared_and_exported():
    from sylber_amd import _lib
    names = {"sylber_dtw_occurrences", "sylber_dtw_occ_workspace_bytes", "sylber_dtw_rerank_occurrences"}
    assert names <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.sylber_dtw_occ_workspace_bytes(3, 8, 5) == 2 * 512 + 1024 + 2 * 256 + 512       # [3][8][5] and [3][4][5] lists, 256-byte pieces
    assert lib.sylber_dtw_occ_workspace_bytes(0, 8, 5) == -1 and lib.sylber_dtw_occ_workspace_bytes(3, 129, 5) == -1
    assert lib.sylber_dtw_occ_workspace_bytes(3, 8, 129) == -1
    # status 1 and a message before any device call
    assert lib.sylber_dtw_occurrences(*([None] * 1 + [1] + [None] * 3 + [1, 1, None, 1, 16, None, 0, 1, None, None, 1] + [None] * 7)) == 1
    assert b"sylber_dtw_occurrences" in lib.sylber_last_error()
    assert lib.sylber_dtw_rerank_occurrences(*([None, 1, None, None, None, 1, None, 1, 16, None, 0, None, 1, None, 1, 1] + [None] * 5)) == 1
    assert b"sylber_dtw_rerank_occurrences" in lib.sylber_last_error()
    # more list entries than the merge indexes: refused with the advice of sylber_dtw_search (the pointers are never followed)
    x = 64
    assert lib.sylber_dtw_occurrences(x, 1, x, x, x, 70000, 1, x, 1, 16, x, 0, 128, x, x, 128, None, None, x, x, x, x, None) == 1
    assert b"use smaller phrase chunks" in lib.sylber_last_error()
    assert lib.sylber_dtw_rerank_occurrences(x, 1, x, x, x, 70000, x, 1, 16, x, 0, x, 128, x, 1, 128, x, x, x, x, None) == 1
    assert b"use smaller phrase chunks" in lib.sylber_last_error()
