"""One lock-step call whose regions differ in which optional outputs they want (ps_score.cpp's output plan), through the raw C ABI:
per reduction kind — point table, support, genotypes, phase — every wanted array of the batched call equals, by bytes, that of a
single call on an AlignData of its own with the same arguments.  The regions are phase_cases' small shapes (a few hundred bases, a
handful of events); a fourth region repeats the first with one more pattern of nulls."""
import copy
import ctypes as C

import numpy as np
import pytest

import phase_cases as PC
from poreseq_amd import _capi

pytestmark = pytest.mark.gpu
NAMES = ("M9_W8", "M65_S1", "skipped_site", "M9_W8")
c_dp, c_i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _arr(shape, dtype, want=True):
    """an output array filled with a byte pattern no result has (every byte of it must be written), or None"""
    if not want:
        return None
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).reshape(-1)[:] = 0xAB
    return a


def _p(a, typ=C.c_void_p):
    return None if a is None else a.ctypes.data_as(typ)


def _ptrs(arrs, typ=C.c_void_p):
    return (typ * len(arrs))(*[_p(a, typ) for a in arrs])


def _i32(v):
    return np.array(list(v), dtype=np.int32)


def _bytes(outs):
    return [None if a is None else a.tobytes() for a in outs]


class _Regions:
    """the shapes NAMES as AlignData and edit lists of the C ABI, twice: `one` for the single calls, `lock` for the lock-step call"""

    def __enter__(self):
        self.api = _capi.load_hip()
        self.cs = [PC.shapes()[n] for n in NAMES]
        self.one = [self.api.align_create(c[0], copy.deepcopy(c[1]), c[2]) for c in self.cs]
        self.lock = [self.api.align_create(c[0], copy.deepcopy(c[1]), c[2]) for c in self.cs]
        self.muts = [self.api.muts_create(c[3]) for c in self.cs]
        self.M = [len(c[3]) for c in self.cs]
        self.E = [len(c[1]) for c in self.cs]
        self.harr = self.api._harr
        return self

    def __exit__(self, *exc):
        for h in self.one + self.lock:
            self.api.align_destroy(h)
        for m in self.muts:
            self.api.muts_destroy(m)


def test_point_tables_wanted_per_region():
    PB = C.POINTER(_capi.PsPointBest)
    wants = [(True, True), (False, True), (True, False), (True, True)]        # (table, best)
    with _Regions() as r:
        n = [len(c[0]) - 4 for c in r.cs]
        make = lambda: [(_arr((n[k], _capi.POINT_SLOTS), np.float64, t), _arr(n[k], _capi.POINT_BEST, b)) for k, (t, b) in enumerate(wants)]
        single, lock = make(), make()
        for k, (t, b) in enumerate(single):
            r.api.check(r.api.lib.ps_point_table(r.one[k], _p(t, c_dp), _p(b, PB), n[k]))
        r.api.check(r.api.lib.ps_batch_point_table(len(NAMES), r.harr(r.lock), _ptrs([o[0] for o in lock], c_dp), _ptrs([o[1] for o in lock], PB),
                                                   np.array(n, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))))
        for k in range(len(NAMES)):
            assert _bytes(lock[k]) == _bytes(single[k]), NAMES[k]


def test_support_scores_wanted_per_region():
    PS = C.POINTER(_capi.PsEditSupport)
    G = [2, 3, 1, 2]
    wants = [True, False, True, False]                                        # scores (the records are required)
    with _Regions() as r:
        grp = [_i32(e % G[k] for e in range(r.E[k] + 1)) for k in range(len(NAMES))]
        make = lambda: [(_arr(r.M[k], np.float64, w), _arr((r.M[k], G[k]), _capi.EDIT_SUPPORT)) for k, w in enumerate(wants)]
        single, lock = make(), make()
        for k, (s, rec) in enumerate(single):
            r.api.check(r.api.lib.ps_score_mutation_support(r.one[k], r.muts[k], G[k], _p(grp[k], c_i32p), _p(s, c_dp), _p(rec, PS)))
        r.api.check(r.api.lib.ps_batch_score_mutation_support(len(NAMES), r.harr(r.lock), r.harr(r.muts), _p(_i32(G), c_i32p), _ptrs(grp, c_i32p),
                                                              _ptrs([o[0] for o in lock], c_dp), _ptrs([o[1] for o in lock], PS)))
        for k in range(len(NAMES)):
            assert _bytes(lock[k]) == _bytes(single[k]), NAMES[k]


def test_genotype_records_scores_and_counts_wanted_per_region():
    PS = C.POINTER(_capi.PsEditSupport)
    G = [2, 3, 1, 2]
    fracs = [[0.5], [0.25, 0.5, 0.75], [], [0.1, 0.9]]
    # (scores, support records, n_cover): records wanted in one region and not the next; without records k_genotype writes the scores
    wants = [(True, True, True), (True, False, True), (False, True, False), (False, False, False)]
    with _Regions() as r:
        grp = [_i32(e % G[k] for e in range(r.E[k] + 1)) for k in range(len(NAMES))]
        fr = [np.array(f + [0.0], dtype=np.float64) for f in fracs]
        nf = [len(f) for f in fracs]
        make = lambda: [(_arr(r.M[k], np.float64, s), _arr((r.M[k], G[k]), _capi.EDIT_SUPPORT, rec), _arr((r.M[k], nf[k] + 1), np.float64),
                         _arr(r.M[k], np.int32, nc)) for k, (s, rec, nc) in enumerate(wants)]
        single, lock = make(), make()
        for k, (s, rec, lik, nc) in enumerate(single):
            r.api.check(r.api.lib.ps_score_mutation_genotypes(r.one[k], r.muts[k], G[k], _p(grp[k], c_i32p), nf[k], _p(fr[k], c_dp), _p(s, c_dp),
                                                              _p(rec, PS), _p(lik, c_dp), _p(nc, c_i32p)))
        r.api.check(r.api.lib.ps_batch_score_mutation_genotypes(
            len(NAMES), r.harr(r.lock), r.harr(r.muts), _p(_i32(G), c_i32p), _ptrs(grp, c_i32p), _p(_i32(nf), c_i32p), _ptrs(fr, c_dp),
            _ptrs([o[0] for o in lock], c_dp), _ptrs([o[1] for o in lock], PS), _ptrs([o[2] for o in lock], c_dp), _ptrs([o[3] for o in lock], c_i32p)))
        for k in range(len(NAMES)):
            assert _bytes(lock[k]) == _bytes(single[k]), NAMES[k]


def test_phase_scores_event_records_and_set_counts_wanted_per_region():
    wants = [(True, True, True), (False, False, True), (True, True, False), (True, False, False)]      # (scores, hap, n_sets)
    with _Regions() as r:
        W, lim, S_ = [c[4] for c in r.cs], [c[5] for c in r.cs], [c[6] for c in r.cs]
        make = lambda: [(_arr(r.M[k], np.float64, s), _arr((r.M[k], W[k]), _capi.EDIT_LINK), _arr(r.M[k], _capi.EDIT_PHASE),
                         _arr((r.E[k], S_[k]), _capi.EVENT_HAP, h), _arr(1, np.int32, ns)) for k, (s, h, ns) in enumerate(wants)]
        single, lock = make(), make()
        for k, (s, link, ph, hap, ns) in enumerate(single):
            r.api.check(r.api.lib.ps_score_mutation_phase(r.one[k], r.muts[k], W[k], lim[k], S_[k], _p(s, c_dp), _p(link), _p(ph), _p(hap), _p(ns, c_i32p)))
        r.api.check(r.api.lib.ps_batch_score_mutation_phase(
            len(NAMES), r.harr(r.lock), r.harr(r.muts), _p(_i32(W), c_i32p), _p(np.array(lim, dtype=np.float64), c_dp), _p(_i32(S_), c_i32p),
            _ptrs([o[0] for o in lock], c_dp), _ptrs([o[1] for o in lock]), _ptrs([o[2] for o in lock]), _ptrs([o[3] for o in lock]),
            _ptrs([o[4] for o in lock], c_i32p)))
        for k in range(len(NAMES)):
            assert _bytes(lock[k]) == _bytes(single[k]), NAMES[k]
