"""The yardstick of the per-edit read support (ps_score_mutation_support), shared by test_support.py (the fallback path on the CPU
checkers) and test_hip_support.py (k_support on the GPU): the definition restated as plain loops over (edit, group, event), run
over the ORACLE's score_mutation_deltas and the ref_align the oracle's AlignData holds after that call.

  span of event e   (int of the first positive ref_align entry, int of the last one); none without a positive entry
  cover(e, m)       edit m is not skipped (start <= L), e has a span and refstart <= start + 1 <= refend
  scores[m]         -1e-6, then += delta[e][m] for every e in order
  support[m][g]     sum = 0.0, then += delta[e][m] for e ascending with group[e] == g; cover / pos / neg count the covering events of
                    g, those with delta > 0 and those with delta < 0

Integer fields are compared for equality, doubles by their bytes."""
import copy
import ctypes as C

import numpy as np

import backends as B
from poreseq_amd import _capi
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import MutationInfo


def edit(start, orig, mut):
    mi = MutationInfo()
    mi.start, mi.orig, mi.mut = int(start), orig, mut
    return mi


def point_list(draft):
    """FindPointMutations' list (cpp/FindMutations.cpp:200-228) as MutationInfo objects"""
    out = []
    for i in range(max(len(draft) - 4, 0)):
        out.append(edit(i, draft[i], ""))
        out += [edit(i, draft[i], b) for b in "ACGT" if b != draft[i]]
        out += [edit(i, "", b) for b in "ACGT"]
    return out


def strands(events):
    return [1 if ev.model.complement else 0 for ev in events]


def oracle_terms(draft, events, params, muts):
    """(starts, delta [E][M] as lists of Python floats, spans [E] of (refstart, refend) or None) from the oracle: muts=None is the
    point list at point_width"""
    api = B.oracle_api()
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), params)
    E = len(events)
    with PSAlign._Data(pa, point_width=muts is None) as d:
        hm = api.find_point_mutations(d.h) if muts is None else api.muts_create(muts)
        try:
            starts = api.muts_export(hm)[0].tolist()
            delta = api.score_mutation_deltas(d.h, hm, E, len(starts)).tolist()
        finally:
            api.muts_destroy(hm)
        spans = []
        for e in range(E):
            n = int(api.lib.ps_align_n_levels(d.h, e))
            ra, rl = np.empty(n), np.empty(n)
            api.check(api.lib.ps_align_get_event_refs(d.h, e, ra.ctypes.data_as(_capi.c_dp), rl.ctypes.data_as(_capi.c_dp)))
            first = last = None
            for v in ra.tolist():
                if v > 0:
                    first = v if first is None else first
                    last = v
            spans.append(None if first is None else (int(first), int(last)))
    return starts, delta, spans


def covers(spans, starts, L, e, m):
    return starts[m] <= L and spans[e] is not None and spans[e][0] <= starts[m] + 1 <= spans[e][1]


def loop(draft, events, params, muts, groups, G, terms=None):
    """(scores float64 [M], support _capi.EDIT_SUPPORT [M, G]) by the definition; terms: oracle_terms' result when the caller has it"""
    starts, delta, spans = oracle_terms(draft, events, params, muts) if terms is None else terms
    E, M, L = len(events), len(starts), len(draft)
    scores = np.zeros(M, dtype=np.float64)
    sup = np.zeros((M, G), dtype=_capi.EDIT_SUPPORT)
    for m in range(M):
        s = -1e-6
        for e in range(E):
            s += delta[e][m]
        scores[m] = s
        for g in range(G):
            acc, cover, pos, neg = 0.0, 0, 0, 0
            for e in range(E):
                if groups[e] != g:
                    continue
                d = delta[e][m]
                acc += d
                if covers(spans, starts, L, e, m):
                    cover += 1
                    pos += d > 0
                    neg += d < 0
            sup[m, g] = (acc, cover, pos, neg, 0)
    return scores, sup


def same(got, want):
    """integer fields equal, doubles byte for byte; either side may carry the scored list as a third entry"""
    gs, gr = np.asarray(got[0], dtype=np.float64), got[1]
    ws, wr = np.asarray(want[0], dtype=np.float64), want[1]
    if gs.shape != ws.shape or gr.shape != wr.shape or gr.dtype != _capi.EDIT_SUPPORT:
        return False
    if gs.tobytes() != ws.tobytes() or np.ascontiguousarray(gr["sum"]).tobytes() != np.ascontiguousarray(wr["sum"]).tobytes():
        return False
    return all(np.array_equal(gr[k], wr[k]) for k in ("cover", "pos", "neg", "reserved"))


def score_bytes(scored):
    return np.array([s.score for s in scored], dtype=np.float64).tobytes()
