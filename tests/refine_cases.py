"""The steps between the ends of Mutate / Refine, shared by test_refine_steps.py (the oracle against the live reference build, on the
CPU) and test_hip_refine_steps.py (the HIP library against the oracle): regions, seed sets, scored edit lists for the greedy pass,
and the step logs that are compared — ScoreAlignments' `likes` vector, the exported list of every FindMutations / ScoreMutations
call, and the mutated-base count, sequence and every event's ref_align / ref_like after every step.

Everything is compared exactly: integers and strings for equality, doubles by their bytes.  Inputs stay inside the reference's
defined domain: no NaN scores, no negative starts."""
import copy

import numpy as np

import backends as B
import tiled_cases as T
from poreseq_amd import _capi, synth
from poreseq_amd.util import DEFAULT_PARAMS, MutationScore

P0 = dict(DEFAULT_PARAMS, verbose=0)
REGIONS = ("work", "wide420", "cap60", "tiled", "inert", "barely")
SPACING = 10          # cpp/MakeMutations.cpp:77
RECURSE_OVER = 10     # cpp/MakeMutations.cpp:142

_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def region(name):
    """(draft, events, params, truth) of a region, made once per process; the events are a fresh copy on every call"""
    def make():
        if name == "work":
            return synth.make_region(300, 6, 9301, B.oracle_swalign, P0) + (dict(P0),)
        if name == "wide420":
            par = dict(P0, realign_width=45.0)
            return synth.make_region(420, 4, 9302, B.oracle_swalign, par) + (par,)
        if name == "cap60":       # a short, bad draft: FindMutations stops at its cap of len(draft) // 3 edits
            return synth.make_region(60, 5, 9303, B.oracle_swalign, P0, draft_error=0.25) + (dict(P0),)
        if name == "tiled":       # reads that cover part of the region, overhang in region-relative coordinates
            L, M, spans, par = T.random_spans(2)
            return T.tiled_region(L, M, spans, 88502, "loader", par) + (par,)
        draft, events, params, truth = region("work")
        if name == "inert":
            events[1].ref_align[:] = 0          # an event without alignment: its Alignment is a no-op
        elif name == "barely":
            events[2].ref_align[40:] = 0        # an event that barely aligns
        else:
            raise KeyError(name)
        return draft, events, truth, params
    draft, events, truth, params = _once(("region", name), make)
    return draft, copy.deepcopy(events), dict(params), truth


def _rand_seq(seed, n):
    return synth.random_sequence(np.random.default_rng(seed), n)


def seed_sets():
    """name -> seed sequences for the `work` region"""
    def make():
        draft, _, _, truth = region("work")
        rng = np.random.default_rng(9310)
        corrupt3 = synth.corrupt(rng, truth, 0.01, 0.01, 0.01)
        with_n = truth[:150] + "N" + truth[151:]
        over = _rand_seq(9311, 60) + truth + _rand_seq(9312, 60)
        sets = {
            "truth": [truth],
            "duplicate": [truth, truth],
            "draft_itself": [draft],                      # no edit may come out: every CUSUM entry is zero
            "no_alignment": ["ACGT" * 6],
            "unrelated": [_rand_seq(9313, 300)],
            "slice": [truth[40:200]],
            "overhang": [over],
            "corrupt3": [corrupt3],
            "with_N": [with_n],
            "tiny": [truth[100:105], truth[200:208]],      # 1 and 4 states
        }
        sets["mixed7"] = [truth, corrupt3, truth, truth[40:200], over, with_n, truth[200:208]]   # an odd count, one duplicate
        return sets
    return _once("seed_sets", make)


def cap_seeds():
    """a dozen 10 %-corrupted seeds for the `cap60` region"""
    def make():
        truth = region("cap60")[3]
        rng = np.random.default_rng(9320)
        return [synth.corrupt(rng, truth, 0.033, 0.034, 0.033) for _ in range(12)]
    return _once("cap_seeds", make)


# ------------------------------------------------------------------------------------------------ scored lists
def scored(start, orig, mut, score):
    m = MutationScore()
    m.start, m.orig, m.mut, m.score = int(start), orig, mut, float(score)
    return m


SIZES = (0, 1, 5, 15, 16, 17, 33, 100, 700)          # 16 / 17 straddle libstdc++'s insertion-sort threshold
PROFILES = ("distinct_neg", "ties_neg", "ties_pos", "all_neg")


def profile_scores(rng, profile, n):
    """n scores: pairwise different with negatives (survivor-only sort), small integers with negatives (whole-list sort), ties
    without a negative, all negative"""
    if profile == "distinct_neg":
        s = np.round(rng.normal(0.0, 5.0, n), 3) + 1e-7 * np.arange(n)       # (the ramp, below one step of the rounding, makes them pairwise different)
        assert n < 10000 and len(set(s.tolist())) == n and (n < 33 or (s < 0).any())
        return s
    if profile == "ties_neg":
        return rng.integers(-3, 6, n).astype(np.float64)
    if profile == "ties_pos":
        return rng.integers(0, 5, n).astype(np.float64)
    return -0.5 * rng.integers(1, 5, n).astype(np.float64)


def random_edits(rng, seq, n, past_end=True):
    """n edits on `seq`: starts over the whole sequence (with past_end now and then len(seq) .. len(seq) + 2), 0-3 bases out (the
    bases that are there; past the end as many as are left), 0-3 bases in"""
    L = len(seq)
    out = []
    for _ in range(n):
        start = int(rng.integers(0, L))
        if past_end and rng.integers(0, 12) == 0:
            start = L - 2 + int(rng.integers(0, 5))
        no, nm = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        orig = seq[start:start + no] if rng.integers(0, 10) else "ACG"[:no]      # (one in ten: a deletion by length, past the end too)
        mut = "".join("ACGT"[i] for i in rng.integers(0, 4, nm))
        out.append((start, orig, mut))
    return out


def random_list(rng, seq, n, profile, past_end=True):
    sc = profile_scores(rng, profile, n)
    return [scored(s, o, m, v) for (s, o, m), v in zip(random_edits(rng, seq, n, past_end), sc)]


def sweep_cases(n_lists, seed):
    """(sequence, profile, list, big) of the zero-event sweep: random sequences of 5 to 400 bases under the four score profiles in
    turn, sizes drawn from SIZES; one list in 21 is big instead: 700 edits or Refine-sized (9 per position).  21 and 4 share no
    factor, so the big lists take the profiles in turn too (the j-th has profile j % 4), each with both sizes (j // 4 % 2)"""
    rng = np.random.default_rng(seed)
    for k in range(n_lists):
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(5, 401))))
        prof = PROFILES[k % 4]
        big = k % 21 == 20
        n = (700, 9 * max(len(seq) - 4, 0))[k // 21 // 4 % 2] if big else int(SIZES[int(rng.integers(0, len(SIZES)))])
        yield seq, prof, random_list(rng, seq, n, prof), big


def big_applied(tally, prof, big, n_bases):
    """counts, per profile, the big lists of a sweep that applied something"""
    if big and n_bases > 0:
        tally[prof] = tally.get(prof, 0) + 1


def every_live_profile_applied_big_lists(tally):
    return all(tally.get(p, 0) > 0 for p in PROFILES if p != "all_neg")


def _point_edits(seq):
    out = []
    for i in range(max(len(seq) - 4, 0)):
        out.append((i, seq[i], ""))
        out += [(i, seq[i], b) for b in "ACGT" if b != seq[i]]
        out += [(i, "", b) for b in "ACGT"]
    return out


def _sub(seq, p):
    """a substitution of base p"""
    return (p, seq[p], "ACGT"[("ACGT".index(seq[p]) + 1) % 4])


def deferred_k(seq, k, at=150, shift_behind=False):
    """one top-scoring substitution at `at` with k positive substitutions inside its spacing, three positive edits far away; with
    shift_behind one of the far ones is an insertion in front of them all, applied after the deferral"""
    near = [p for p in range(at - 8, at + 10) if p != at][:k]
    assert len(near) == k
    lst = [scored(*_sub(seq, at), 100.0)] + [scored(*_sub(seq, p), 50.0 - i) for i, p in enumerate(near)]
    lst += [scored(*_sub(seq, 20), 9.0), scored(*_sub(seq, 250), 8.0)]
    lst.append(scored(60, "", "GT", 7.0) if shift_behind else scored(*_sub(seq, 60), 7.0))
    return lst


def greedy_lists():
    """name -> scored list for MakeMutations on the `work` region's draft"""
    def make():
        seq = region("work")[0]
        L = len(seq)
        out = {}
        for pi, prof in enumerate(PROFILES):
            for n in SIZES:
                out["%s_%d" % (prof, n)] = random_list(np.random.default_rng([9400, pi, n]), seq, n, prof)
            pts = _point_edits(seq)     # a Refine-sized list: 9 per position
            sc = profile_scores(np.random.default_rng(9390 + pi), prof, len(pts))
            out["%s_refine" % prof] = [scored(s, o, m, v) for (s, o, m), v in zip(pts, sc)]
        a = _sub(seq, 100)
        out["same_edit_twice"] = [scored(*a, 2.5), scored(*a, 2.5), scored(*_sub(seq, 200), 1.0)]
        # scores of exactly 0.0 and -0.0 inside the spacing of an applied insertion: applied, never deferred, still shifted
        out["zero_scores"] = [scored(100, "", "GGG", 3.0), scored(*_sub(seq, 104), 0.0), scored(*_sub(seq, 97), -0.0),
                              scored(*_sub(seq, 108), -0.0), scored(*_sub(seq, 30), 0.0)]
        for gap in (9, 10, 11):      # max(start) - min(start + len(mut)) of two positive edits
            out["spacing_%d" % gap] = [scored(*_sub(seq, 100), 2.0), scored(*_sub(seq, 101 + gap), 1.0)]
        ins, dele = (100, "", "ACGTACGTACGT"), (100, seq[100:103], "")
        for nm, (ed, first) in {"ins": (ins, 100), "del": (dele, 103)}.items():     # an edit at start_i + len(orig_i) and one base before it
            out["shift_%s_at" % nm] = [scored(*ed, 5.0), scored(*_sub(seq, first), 0.0)]
            out["shift_%s_before" % nm] = [scored(*ed, 5.0), scored(*_sub(seq, first - 1), 0.0)]
        out["deferred_behind_applied"] = deferred_k(seq, 11, shift_behind=True)
        out["deferred_10"] = deferred_k(seq, 10)
        out["deferred_11"] = deferred_k(seq, 11)
        out["start_eq_len"] = [scored(L, "", "AC", 3.0), scored(0, "", "GG", 4.0)]
        out["start_gt_len"] = [scored(L + 3, "A", "C", 2.0), scored(*_sub(seq, 50), 1.0)]
        out["deletion_past_end"] = [scored(L - 2, "ACGTA", "", 1.0)]
        out["insertion_at_0"] = [scored(0, "", "TTAGC", 1.0), scored(*_sub(seq, 5), 0.5)]
        return out
    return _once("greedy_lists", make)


RECURSING = ("deferred_11", "deferred_behind_applied")          # more than ten deferred: re-scored and recursed on
NO_DEFERRAL = ("same_edit_twice", "zero_scores", "spacing_10", "spacing_11", "shift_ins_at", "shift_ins_before", "shift_del_at",
               "shift_del_before", "start_eq_len", "start_gt_len", "deletion_past_end", "insertion_at_0")


def plain_make_mutations(seq, muts):
    """cpp/MakeMutations.cpp:74-146 on an AlignData without events, for lists whose surviving scores are pairwise different (then
    sorted() by -score is std::sort's order): -> (mutated bases, sequence).  Re-scoring without events gives -1e-6 everywhere, so
    the recursion applies nothing."""
    muts = sorted(([m.start, m.orig, m.mut, m.score] for m in muts if not m.score < 0), key=lambda m: -m[3])
    nb = 0
    for i, (si, oi, mi, sci) in enumerate(muts):
        if sci < 0:
            continue                                              # deferred: handed to the next round
        if si < len(seq):                                         # Sequence(original, mut), cpp/Sequence.h:37-59
            seq = seq[:si] + mi + seq[si + len(oi):]
        nb += max(len(oi), len(mi))
        for m in muts[i + 1:]:
            lo, hi = max(si, m[0]), min(si + len(mi), m[0] + len(m[2]))
            if lo < hi + SPACING and m[3] > 0:
                m[3] = -1.0                                       # overlaps with the spacing: later, and NOT shifted now
                continue
            if m[0] >= si + len(oi):
                m[0] += len(mi) - len(oi)
    return nb, seq


# ------------------------------------------------------------------------------------------------ step logs
def listing(api, hm):
    start, orig, mut, score = api.muts_export(hm)
    return start.tolist(), orig, mut, score.tobytes()


def state(api, h, n_events):
    """(sequence, [(ref_align bytes, ref_like bytes)] per event) of an AlignData as it is now"""
    refs = []
    for e in range(n_events):
        n = int(api.lib.ps_align_n_levels(h, e))
        ra, rl = np.empty(n), np.empty(n)
        api.check(api.lib.ps_align_get_event_refs(h, e, ra.ctypes.data_as(_capi.c_dp), rl.ctypes.data_as(_capi.c_dp)))
        refs.append((ra.tobytes(), rl.tobytes()))
    return api.align_sequence(h), refs


def rounds(api, draft, events, params, seeds, n_rounds=3):
    """the log of n_rounds of find_mutations -> score_mutations -> make_mutations on ONE handle, as poreseqcpp.Mutate runs them
    (without its stop at zero mutated bases), then ps_align_new_call and one more find_mutations: [(label, what the step returned,
    state after it)]"""
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), params)
    log = []
    try:
        for r in range(n_rounds):
            hm = api.find_mutations(h, seeds)
            try:
                log.append(("find %d" % r, listing(api, hm), state(api, h, E)))
                hs = api.score_mutations(h, hm)
            finally:
                api.muts_destroy(hm)
            try:
                log.append(("score %d" % r, listing(api, hs), state(api, h, E)))
                nb = api.make_mutations(h, hs)
            finally:
                api.muts_destroy(hs)
            log.append(("make %d" % r, nb, state(api, h, E)))
        api.check(api.lib.ps_align_new_call(h, int(params["scoring_width"])))
        hm = api.find_mutations(h, seeds)
        try:
            log.append(("find after new_call", listing(api, hm), state(api, h, E)))
        finally:
            api.muts_destroy(hm)
    finally:
        api.align_destroy(h)
    return log


def apply_list(api, draft, events, params, muts):
    """ps_make_mutations of a scored list on a fresh AlignData -> (mutated bases, state after)"""
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        hm = api.muts_create(muts, with_scores=True)
        try:
            nb = api.make_mutations(h, hm)
        finally:
            api.muts_destroy(hm)
        return nb, state(api, h, len(events))
    finally:
        api.align_destroy(h)


def point_listing(api, seq):
    """FindPointMutations' list on a sequence without events"""
    h = api.align_create(seq, [], P0)
    try:
        hm = api.find_point_mutations(h)
        try:
            return listing(api, hm)
        finally:
            api.muts_destroy(hm)
    finally:
        api.align_destroy(h)


def likes_twice(api, draft, events, params):
    """(scores, likes) of score_alignments(likes_len = len(draft)), then a second call on the same handle into a buffer that holds
    the first result plus a constant -> (scores bytes, likes bytes, second scores bytes, second buffer bytes, the buffer before)"""
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        sc, lk = api.score_alignments(h, E, likes_len=len(draft))
        buf = lk + 0.375
        before = buf.copy()
        sc2, lk2 = api.score_alignments(h, E, likes=buf)
        assert lk2 is buf
        return sc.tobytes(), lk.tobytes(), sc2.tobytes(), buf.tobytes(), before
    finally:
        api.align_destroy(h)


def likes_per_event(api, draft, events, params):
    """[(likes of the first call, likes of the second call)] of every event ALONE on a handle of its own, each call into zeros: the
    terms that ScoreAlignments adds into the caller's vector, event by event in order (cpp/MakeMutations.cpp:168-189)"""
    out = []
    for ev in events:
        h = api.align_create(draft, [copy.deepcopy(ev)], params)
        try:
            out.append(tuple(api.score_alignments(h, 1, likes_len=len(draft))[1] for _ in range(2)))
        finally:
            api.align_destroy(h)
    return out


def fold(start, terms):
    """((start + terms[0]) + terms[1]) + ...: the additions in the order ScoreAlignments makes them"""
    acc = np.array(start, dtype=np.float64)
    for t in terms:
        acc = acc + t
    return acc


def first_difference(got, want):
    """label of the first step of two logs that differs, or None"""
    for g, w in zip(got, want):
        if g != w:
            what = "result" if g[1] != w[1] else ("sequence" if g[2][0] != w[2][0] else "event refs")
            return "%s: %s" % (g[0], what)
    return None if len(got) == len(want) else "log lengths %d / %d" % (len(got), len(want))


_oracle = {}


def oracle_once(key, make):
    """an oracle result computed once per session and handed out unchanged (callers must not write into it)"""
    if key not in _oracle:
        _oracle[key] = make()
    return _oracle[key]
