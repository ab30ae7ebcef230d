"""Caller-written ref_align arrays on the CPU (tests/ref_cases.py): the oracle's bands, its number of kept Viterbi positions and the emission
rows that one read alone contributes to against the plain restatement of cpp/EventData.h:110-204, the oracle against the live reference build on every API result, and the preconditions that
keep the crafted arrays from going stale (each family is asserted to reach the branch it was written for).  The HIP path is held to
the same oracle in test_hip_ref_tables.py."""
import copy

import numpy as np
import pytest

import backends as B
import ref_cases as RC

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (the reference sources are not here)")
cases = pytest.mark.parametrize("name", RC.ALL_CASES, ids=RC.case_id)


# ---- the restatement on arrays small enough to do by hand ------------------------------------------------------------------------
def test_restatement_by_hand():
    t = RC.ref_tables([5, 0, 0, 8, 0, 10, 0])                  # the hole behind level 0 stays; the second one is interpolated
    assert t.ref_index == [5.0, 0.0, 0.0, 8.0, 9.0, 10.0, 11.0] and (t.refstart, t.refend) == (5, 10)
    assert t.sic and t.interpolated == {4} and t.holes == [(1, 3), (4, 5)]
    assert [t.getrefstate(j) for j in (0, 5, 6, 9, 11, 12)] == [0, 3, 3, 4, 6, 7]       # the bisection never looks at level 0
    assert t.getrefstates(9) == [4] and t.getrefstates(8) == [3, ] and t.getrefstates(0) == [1] and t.getrefstates(7) == []
    t = RC.ref_tables([0, 0, 7, 0])                            # one aligned level: 0 / 0
    assert t.ref_index[2] == 7.0 and all(x != x for k, x in enumerate(t.ref_index) if k != 2) and t.has_nan()
    assert t.getrefstate(3) == 0 and t.getrefstate(9) == 3    # NaN < j is false: the walk goes left wherever it meets one
    t = RC.ref_tables([0, -1, float("nan")])
    assert t.ref_index is None and (t.refstart, t.refend) == (-1, -1) and t.getrefstate(3) == 0 and t.getrefstates(-1) == []
    t = RC.ref_tables([0.25, 3.5, 3.0, 2.0])                   # column 0, a fraction, back steps
    assert (t.refstart, t.refend) == (0, 2) and t.unsorted() and t.getrefstates(3) == [2, 3] and t.getrefstates(2) == [3]
    m = RC.band_mask([0, 2, 3, 0], 4, 3, 1, 0)
    assert bool(m[:, 0].all()) and m[:, 1].tolist() == [False, True, True, False, False] and m[:, 3].tolist() == [False, True, True, True, False]
    assert RC.band_mask([0, 2, 3, 0], 4, 3, 1, 1)[:, 1].tolist() == [False, False, True, True, True]      # n0 - getrefstate(3) + 1 = 3


def test_level_counts_and_chunks():
    assert [RC.chunk_of(n) for n in (0, 1, 2, 255, 256, 257, 513, 1025)] == [0, 1, 1, 1, 1, 2, 3, 5]
    seen = set()
    for name, (draft, events, par) in RC.crafted().items():
        counts = RC.FAMILIES[name][1]
        assert tuple(ev.mean.size for ev in events) == counts and (len(set(counts)) >= 2 or name in RC.ONE_READ), name
        assert all(ev.stdv.size == ev.ref_align.size == ev.ref_like.size == n for ev, n in zip(events, counts)), name
        assert len(draft) <= 1200 and len(events) <= 3
        seen.update(counts)
    assert seen == {0, 1, 2, 255, 256, 257, 513, 1025}
    for s in RC.RANDOM_SEEDS:
        draft, events, par = RC.random_case(s)
        assert 2 <= len(events) <= 3 and all(1 <= ev.mean.size <= 600 for ev in events)


def test_levels_cut():
    draft, events = RC.base_region((40, 30), 9001)
    whole = copy.deepcopy(events)
    RC.levels_cut(events, 7)
    for ev, w in zip(events, whole):
        for k in ("mean", "stdv", "ref_align", "ref_like"):
            assert getattr(ev, k).size == 7 and np.array_equal(getattr(ev, k), getattr(w, k)[:7]) and getattr(ev, k).flags.c_contiguous


def test_families_reach_what_they_claim():
    made = RC.crafted()
    for attr, names in RC.REACH.items():
        for name in names:
            tabs = [RC.ref_tables(ev.ref_align) for ev in made[name][1]]
            flags = [getattr(t, attr)() if callable(getattr(t, attr)) else getattr(t, attr) for t in tabs]
            assert any(flags), (attr, name)
    # the hole behind level 0 is as the caller wrote it, and the later hole is not
    for ev in made["sic_hole"][1]:
        t, h = RC.ref_tables(ev.ref_align), 1 if ev is made["sic_hole"][1][0] else 3 * RC.chunk_of(ev.mean.size) + 1
        assert t.sic and t.ref_index[1:h + 1] == [0.0] * h and len(t.interpolated) >= 2 and t.holes[0] == (1, h + 1)
    # every hole of chunk_holes is interpolated and lies on the chunks as described
    for ev in made["chunk_holes"][1]:
        t, c = RC.ref_tables(ev.ref_align), RC.chunk_of(ev.mean.size)
        want = [(10 * c, 11 * c), (20 * c - 1, 24 * c + 1), (30 * c + c // 2 if c > 1 else 29, 31 * c), (40 * c, 40 * c + max(1, c // 2))]
        assert all(h in t.holes for h in want) and not t.sic and t.whole_chunk_hole(), t.holes
        assert all(j in t.interpolated for a, b in want for j in range(a, b))
    for name, first_in_last, last_in_first in (("late_first", True, False), ("early_last", False, True)):
        for ev in made[name][1]:
            t, c, n = RC.ref_tables(ev.ref_align), RC.chunk_of(ev.mean.size), ev.mean.size
            assert (t.first >= ((n - 1) // c) * c) == first_in_last and (t.last < c) == last_in_first, name
    for name in ("single_at_0", "single_mid", "single_last"):
        for ev in made[name][1]:
            assert int(np.count_nonzero(ev.ref_align > 0)) == 1, name
    for ev in made["two_equal"][1]:
        on = np.flatnonzero(ev.ref_align > 0)
        t = RC.ref_tables(ev.ref_align)
        assert on.size == 2 and ev.ref_align[on[0]] == ev.ref_align[on[1]] and t.ref_index == [ev.ref_align[on[0]]] * ev.mean.size
    for ev in made["markers"][1]:
        t = RC.ref_tables(ev.ref_align)
        assert t.ref_index[1] == -1.0 and t.ref_index[4] != t.ref_index[4] and t.has_nan() and t.sic
        a = ev.mean.size // 3
        assert all(j in t.interpolated for j in range(a, a + 6)) and np.isnan(ev.ref_align[a + 2])
        assert t.last == ev.mean.size - 13 and not any(x != x for x in t.ref_index[t.last:])      # the tail is the line, not the markers
    for ev in made["fractional"][1]:
        assert int(np.count_nonzero(ev.ref_align != np.floor(ev.ref_align))) >= 30
    for ev in made["column0"][1]:
        assert RC.ref_tables(ev.ref_align).refstart == 0
    draft, events, _ = made["past_end"]
    assert [RC.ref_tables(ev.ref_align).refend for ev in events][1:] == [20000, 20000] and all(ev.ref_align.max() <= 20000 for ev in events)
    assert RC.ref_tables(events[0].ref_align).refend > len(draft) + 300
    for ev in made["long_run"][1]:
        a = ev.mean.size // 3
        assert np.all(ev.ref_align[a:a + 80] == ev.ref_align[a]) and ev.ref_align[a] > 0
    assert RC.ref_tables(made["all_unaligned"][1][1].ref_align).ref_index is None
    t0, t1 = (RC.ref_tables(ev.ref_align) for ev in made["unaligned_markers"][1][:2])
    assert t0.ref_index is None and t1.find(-1) == 1
    # Viterbi hits on interpolated levels; the walk that starts at position -1 keeps it
    for name in RC.INTERP_HIT:
        events = made[name][1]
        tabs = [RC.ref_tables(ev.ref_align) for ev in events]
        hits = [(e, first) for _, here in RC.viterbi_positions(events) for e, _, _, first in here if first in tabs[e].interpolated]
        assert len(hits) >= 2, name
    assert RC.viterbi_positions(made["unaligned_markers"][1])[0][0] == -1
    # the read of 0 levels: no tables, no band beyond the blank column, and the walk of its region starts at -1 and keeps positions
    empty = made["empty_read"][1][0]
    t = RC.ref_tables(empty.ref_align)
    assert empty.mean.size == 0 and t.ref_index is None and t.refstart == -1 and t.getrefstate(5) == 0 and t.getrefstates(5) == []
    assert RC.band_mask(t, 0, 7, 20, 0).tolist() == [[True] + [False] * 7]
    walk = RC.viterbi_positions(made["empty_read"][1])
    assert len(walk) > 200
    assert all(len(here) == 1 for _, here in RC.viterbi_positions(made["one_read"][1]))


# ---- the oracle against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", RC.WIDTHS[:2])
@cases
def test_oracle_bands_equal_the_restatement(name, W):
    """the NaN pattern of the oracle's debug_fill, forward and backward, every event"""
    draft, events, par = RC.case(name)
    par = RC.with_width(par, W)
    C = len(draft) - 4
    for e, ev in enumerate(events):
        t = RC.ref_tables(ev.ref_align)
        for d in (0, 1):
            main = RC.fill_tables(B.oracle_api(), draft, events, par, e, d)[0]
            want = RC.band_mask(t, ev.mean.size, C, W, d)
            got = ~np.isnan(main)
            if not np.array_equal(got, want):
                cols = np.flatnonzero((got != want).any(axis=0))
                raise AssertionError("event %d, direction %d: first differing column %d" % (e, d, cols[0]))


ALONE = ("one_read", "sic_hole", "chunk_holes", "markers", "past_end", "empty_read", "unaligned_markers")


def viterbi_want(name):
    return RC.once(("positions", name), lambda: RC.viterbi_positions(RC.case(name)[1]))


@cases
def test_oracle_viterbi_positions_equal_the_restatement(name):
    """The number of kept positions, and the emission row of every position that one event alone contributes to (debug_viterbi does
    not hand out the positions themselves: with one contributor the row is a function of the levels the restatement picked, so
    these rows pin position, hit and walk; `one_read` has no other kind of position, and the families named in ALONE must have some)"""
    draft, events, par = RC.case(name)
    want = viterbi_want(name)
    got = RC.viterbi_tables(B.oracle_api(), draft, events, par, 1, len(want) + 4)
    assert got["T"] == len(want)
    alone = [(t, here[0]) for t, (_, here) in enumerate(want) if len(here) == 1]
    assert alone or name not in ALONE
    if name in RC.ONE_READ:
        assert len(alone) == len(want) > 200
    for t, (e, lvl, sd, _) in alone:
        assert np.array_equal(got["obs"][t], RC.emission_row(events[e].model, lvl, sd)), (t, e)


# ---- the oracle against the live reference ---------------------------------------------------------------------------------------------
def api_log(cls, draft, events, params, viterbi):
    """ScoreEvents, ScorePoints, ScoreMutations of 20 edits, Mutate('viterbi', 1), Mutate('self', 1), Refine, final refs.
    viterbi=False leaves the Viterbi call out: where the walk keeps no position the reference's back-trace starts from a table
    that holds the start vector alone and reads the states of a path without positions (cpp/Viterbi.cpp:373-426: it crashes)."""
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), params)
    log = [mk().ScoreEvents(), [(s.start, s.orig, s.mut, s.score) for s in mk().ScorePoints()],
           [s.score for s in mk().ScoreMutations(RC.edits(draft))]]
    B.reset_rand()
    pa = mk()
    if viterbi:
        log += [pa.Mutate(seqs="viterbi", reps=1), pa.sequence]
    log += [pa.Mutate(reps=1), pa.sequence]
    log += [pa.Refine(), pa.sequence]
    return log, RC.refs(pa)


# cases whose walk keeps no position.  all_unaligned: read 1 puts the start at -1, where it alone counts as aligned (refstart =
# refend = -1) and nothing is found; at 0 no read is aligned (the live reads start at column 1 or later) and the walk ends.
NO_POSITIONS = ("all_unaligned",)


def test_walks_without_positions_return_no_sequences():
    for name in NO_POSITIONS:
        draft, events, par = RC.case(name)
        assert viterbi_want(name) == []
        pa = B.make_pa(B.OraclePSAlign, draft, events, par)
        assert pa.Mutate(seqs="viterbi", reps=1) == 0 and pa.sequence == draft


@need_ref
@pytest.mark.parametrize("W", RC.WIDTHS[:2])
@cases
def test_oracle_equals_the_reference_build(name, W):
    draft, events, par = RC.case(name)
    par = RC.with_width(par, W)
    T = len(viterbi_want(name))
    assert T > 0 or name in NO_POSITIONS, "the walk keeps no position: not a case for the reference"
    got, want = api_log(B.OraclePSAlign, draft, events, par, T > 0), api_log(B.RefPSAlign, draft, events, par, T > 0)
    for k, (x, y) in enumerate(zip(got[0], want[0])):
        assert x == y or (np.asarray(x).dtype.kind == "f" and np.array_equal(x, y, equal_nan=True)), k
    assert RC.same_arrays(got[1], want[1])


# ---- out-of-range entries ------------------------------------------------------------------------------------------------------------
OUT_OF_RANGE = (2147483648.0, 1e12, float("inf"))


def out_of_range_case(v):
    draft, events, par = RC.case("untouched")
    events[1].ref_align[17] = v
    return draft, events, par


@pytest.mark.parametrize("v", OUT_OF_RANGE)
def test_oracle_refuses_viterbi_on_entries_not_below_2_31(v):
    from poreseq_amd._capi import PoreseqError
    api = B.oracle_api()
    draft, events, par = out_of_range_case(v)
    h = api.align_create(draft, copy.deepcopy(events), par)
    try:
        for call in (lambda: api.viterbi_mutate(h, 16, *RC.VIT, 0), lambda: api.debug_viterbi([h], 64, 0, *RC.VIT)):
            with pytest.raises(PoreseqError) as err:
                call()
            assert "event 1, level 17" in str(err.value) and "2^31" in str(err.value), str(err.value)
        with pytest.raises(PoreseqError) as err:
            api.batch_viterbi_mutate([h], [None], 16, *RC.VIT)
        assert "ps_batch_viterbi_mutate: region 0: event 1, level 17" in str(err.value), str(err.value)
        assert len(api.score_alignments(h, len(events))) == len(events)       # the DP takes any double, and the handle lives on
    finally:
        api.align_destroy(h)
    draft, events, par = RC.case("untouched")
    h = api.align_create(draft, copy.deepcopy(events), par)                   # the library is usable afterwards
    try:
        assert len(api.viterbi_mutate(h, 16, *RC.VIT, 0)) == 16
    finally:
        api.align_destroy(h)
