"""CPU tests of the steps between the ends of Mutate / Refine (refine_cases.py): the ORACLE against the live reference build —
ScoreAlignments' `likes` vector and its accumulation, the list of every FindMutations / ScoreMutations call and the state after
every step of three rounds on one handle, FindPointMutations' list, and MakeMutations on crafted and random scored lists, with
events and as pure list logic on an AlignData without events — and the library's own host code for the same steps, compiled
stand-alone: its greedy pass (ps_greedy.h) against the checkers and its block-maxima extraction (ps_extract.h) against a rescan.

The oracle-against-reference tests skip when oracle/_ref/libps_ref.so is absent, as test_oracle.py's do."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import refine_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (reference tree absent)")


# ------------------------------------------------------------------------------------------------ likes
@need_ref
@pytest.mark.parametrize("name", R.REGIONS)
def test_likes_vector_and_its_accumulation(name):
    draft, events, par, _ = R.region(name)
    orc = R.likes_twice(B.oracle_api(), draft, events, par)
    ref = R.likes_twice(B.ref_api(), draft, events, par)
    assert orc[:4] == ref[:4]
    # "accumulated into": every event's vector is added onto what the buffer holds, event by event.  The events' own vectors come
    # from handles that hold one event each (the second call runs on the refs the first one left, so it has vectors of its own).
    # This is checked on the oracle's vectors alone: the reference, above, and the HIP library, in test_hip_refine_steps.py, are
    # held to it through the equality of their bytes with the oracle's
    terms = R.likes_per_event(B.oracle_api(), draft, events, par)
    first = np.frombuffer(orc[1])
    assert first.tobytes() == R.fold(np.zeros(len(draft)), [t[0] for t in terms]).tobytes()
    assert orc[3] == R.fold(orc[4], [t[1] for t in terms]).tobytes()
    assert first.any() and orc[3] != orc[4].tobytes()


def test_a_likes_buffer_shorter_than_the_sequence_is_refused():
    from poreseq_amd._capi import PoreseqError
    api = B.oracle_api()
    draft, events, par, _ = R.region("work")
    h = api.align_create(draft, events, par)
    try:
        for kw in (dict(likes=np.zeros(len(draft) - 1)), dict(likes_len=len(draft) - 1)):
            with pytest.raises(PoreseqError, match="likes has"):
                api.score_alignments(h, len(events), **kw)
        api.score_alignments(h, len(events), likes=np.zeros(len(draft) + 3))       # longer is fine
    finally:
        api.align_destroy(h)


# ------------------------------------------------------------------------------------------------ FindMutations rounds
def _rounds_equal(draft, events, par, seeds):
    orc = R.rounds(B.oracle_api(), draft, events, par, seeds)
    ref = R.rounds(B.ref_api(), draft, events, par, seeds)
    assert R.first_difference(orc, ref) is None
    return orc


@need_ref
@pytest.mark.parametrize("name", sorted(R.seed_sets()))
def test_three_rounds_step_by_step(name):
    draft, events, par, _ = R.region("work")
    log = _rounds_equal(draft, events, par, R.seed_sets()[name])
    if name == "draft_itself":
        assert log[0][1][0] == [] and log[2][1] == 0        # no edit, nothing applied
    if name == "truth":
        assert len(log[0][1][0]) > 3 and log[2][1] > 0      # the case does something


@need_ref
@pytest.mark.parametrize("name", ["wide420", "tiled", "inert", "barely"])
def test_three_rounds_on_the_other_regions(name):
    draft, events, par, truth = R.region(name)
    _rounds_equal(draft, events, par, [truth, truth[30:150]])


@need_ref
def test_list_stops_at_the_cap():
    draft, events, par, _ = R.region("cap60")
    log = _rounds_equal(draft, events, par, R.cap_seeds())
    assert len(log[0][1][0]) == len(draft) // 3          # exactly the cap: the case cannot silently stop reaching it


@need_ref
@pytest.mark.parametrize("seq", ["ACGT", "ACGTA", "GATTACAGATNACAGGATTACA"])
def test_point_list(seq):
    orc, ref = R.point_listing(B.oracle_api(), seq), R.point_listing(B.ref_api(), seq)
    assert orc == ref
    assert len(orc[0]) == sum(8 + (c not in "ACGT") for c in seq[:max(len(seq) - 4, 0)])   # an N has four substitutions


# ------------------------------------------------------------------------------------------------ greedy pass
@need_ref
@pytest.mark.parametrize("name", sorted(R.greedy_lists()))
def test_greedy_pass_with_events(name):
    draft, events, par, _ = R.region("work")
    muts = R.greedy_lists()[name]
    orc = R.apply_list(B.oracle_api(), draft, events, par, muts)
    ref = R.apply_list(B.ref_api(), draft, events, par, muts)
    assert orc == ref
    if name in ("spacing_10", "spacing_11"):
        assert orc[0] == 2                   # both applied
    if name == "spacing_9":
        assert orc[0] == 1                   # the second one deferred (and, alone, dropped)
    if name in ("start_eq_len", "start_gt_len"):
        assert orc[0] == 4 if name == "start_eq_len" else orc[0] == 2      # counted although the sequence is only copied


@need_ref
def test_greedy_pass_as_list_logic():
    """no events: re-scoring gives -1e-6 everywhere.  Oracle against reference on a few thousand lists, and for the tie-free
    profile against the plain statement of the defer / shift rules (refine_cases.plain_make_mutations)"""
    orc, ref = B.oracle_api(), B.ref_api()
    applied = plain = 0
    big = {}
    for seq, prof, muts, is_big in R.sweep_cases(2400, 9500):
        a = R.apply_list(orc, seq, [], R.P0, muts)
        b = R.apply_list(ref, seq, [], R.P0, muts)
        assert a == b, (seq, prof, len(muts))
        applied += a[0] > 0
        R.big_applied(big, prof, is_big, a[0])
        if prof == "distinct_neg":
            assert R.plain_make_mutations(seq, muts) == (a[0], a[1][0]), (seq, len(muts))
            plain += 1
    assert applied > 1000 and plain == 600
    assert R.every_live_profile_applied_big_lists(big), big


def test_plain_statement_on_the_hand_written_lists():
    """the plain statement agrees with the oracle on the crafted lists without tied survivors, on the `work` draft without events"""
    seq = R.region("work")[0]
    for name in ("spacing_9", "spacing_10", "spacing_11", "shift_ins_at", "shift_ins_before", "shift_del_at", "shift_del_before",
                 "deferred_10", "deferred_11", "deferred_behind_applied", "start_eq_len", "start_gt_len", "deletion_past_end", "insertion_at_0"):
        muts = R.greedy_lists()[name]
        nb, st = R.apply_list(B.oracle_api(), seq, [], R.P0, muts)
        assert R.plain_make_mutations(seq, muts) == (nb, st[0]), name


# ------------------------------------------------------------------------------------------------ the library's host code
def _native(name, args, libs=()):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, name)
        subprocess.check_call(["g++", "-O2", os.path.join(HERE, "native", name + ".cpp"), "-o", exe] + list(libs))
        return subprocess.run([exe] + args, stdout=subprocess.PIPE, timeout=300).stdout.decode()


def _counts(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)}


def test_block_maxima_extraction_equals_the_rescan():
    out = _native("extract_check", ["4000"])
    assert out.strip().endswith("mismatches=0"), out
    counts = _counts(out.strip().splitlines()[-2])
    assert sorted(counts) == sorted(["tie_blocks", "tie_seeds", "run_span", "fill_span", "no_zero_before", "no_zero_after", "short_vec",
                                     "empty_vec", "no_seeds"]), out
    assert all(v > 0 for v in counts.values()), out          # every situation the block maxima could get wrong did occur


@pytest.mark.parametrize("checker", ["oracle", "reference"])
def test_library_greedy_pass_equals_the_checkers(checker):
    if checker == "reference" and not B.have_ref():
        pytest.skip("oracle/_ref not built (reference tree absent)")
    B.build_oracle()
    out = _native("greedy_check", [B.ORACLE_SO if checker == "oracle" else B.REF_SO, "3000"], libs=["-ldl"])
    assert out.strip().endswith("mismatches=0"), out
    counts = _counts(out.strip().splitlines()[-2])
    assert all(counts[k] > 0 for k in ("deferred", "recursed", "tied", "past_end", "big_distinct_neg", "big_ties_neg", "big_ties_pos")), out
