"""Shared by test_point_table.py (CPU checkers) and test_hip_point_table.py (the HIP library): what a point-edit table is held to."""
import numpy as np

import backends as B


def check_against_vector(z, res):
    """`res` = PointTable() of fixture z: the non-NaN entries, read row by row (FindPointMutations' order), are the reference's
    ScorePoints scores; the NaN slots are the substitutions by the base itself; margin / slot / n_positive are numpy's on that vector"""
    table, margin, slot, npos = res
    seq, want = str(z["sequence"]), z["ScorePoints_score"]
    n = len(seq) - 4
    assert table.shape == (n, 9) and table.dtype == np.float64
    mask = np.zeros((n, 9), dtype=bool)
    for p in range(n):
        mask[p, 1 + "ACGT".index(seq[p])] = True
    assert np.array_equal(np.isnan(table), mask)
    assert np.array_equal(table[~mask], want)
    rows = want.reshape(n, 8)                       # (every base of these fixtures is one of ACGT: 8 edits per position)
    assert np.array_equal(margin, rows.max(axis=1))
    first = np.array([int(np.flatnonzero(~mask[p])[np.argmax(rows[p])]) for p in range(n)])
    assert np.array_equal(slot, first) and slot.dtype == np.int32
    assert np.array_equal(npos, (rows > 0).sum(axis=1)) and npos.dtype == np.int32


def same(a, b):
    """two (table or None, margin, slot, n_positive) results are equal: tolerance 0, NaN slots compared as a mask"""
    if (a[0] is None) != (b[0] is None):
        return False
    if a[0] is not None and not (a[0].shape == b[0].shape and np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
                                 and np.array_equal(a[0][~np.isnan(a[0])], b[0][~np.isnan(b[0])])):
        return False
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def oracle_table(draft, events, params):
    """the oracle's fallback PointTable (the literal construction from its scored list) of a region; the inputs are not modified"""
    import copy
    return B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), params).PointTable()
