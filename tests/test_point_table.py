"""The per-position point-edit table (`PSAlign.PointTable`, include/poreseq_hip.h: ps_point_table) and what is built on it — consensus
base qualities, `consensus.variant_points` — on the CPU checkers, which lack the entry point and so run the literal construction that
defines the result (poreseqcpp.point_table_from_list).  All comparisons are exact; NaN slots are compared as a mask.  The HIP path
is held to the same vectors in test_hip_point_table.py."""
import copy
import io

import numpy as np
import pytest

import backends as B
import golden_util as G
from point_cases import check_against_vector
from poreseq_amd import _capi, synth
from poreseq_amd.consensus import consensus_region, variant_points, variant_region
from poreseq_amd.util import DEFAULT_PARAMS, phred_from_margin, write_fastq

SCORE_CASES = ["score_L300_E5", "score_L240_E4_narrow"]
NEW = ("ps_point_table", "ps_batch_point_table")
P0 = dict(DEFAULT_PARAMS, verbose=0)


def checkers():
    return [B.OraclePSAlign] + ([B.RefPSAlign] if B.have_ref() else [])


@pytest.mark.parametrize("name", SCORE_CASES)
def test_fallback_point_table_equals_the_reference_vector(name):
    z = G.load(name)
    for cls in checkers():
        pa = G.make(cls, z)
        before = (pa.sequence, [ev.ref_align.copy() for ev in pa.events])
        res = pa.PointTable()
        check_against_vector(z, res)
        lean = pa.PointTable(table=False)
        assert lean[0] is None and all(np.array_equal(a, b) for a, b in zip(lean[1:], res[1:]))
        assert pa.sequence == before[0] and all(np.array_equal(a.ref_align, b) for a, b in zip(pa.events, before[1]))


def test_first_maximum_and_other_characters_in_the_literal_construction():
    from poreseq_amd.poreseqcpp import point_table_from_list
    # position 0 'N': nine edits, a tie between the deletion and an insertion; position 1 'C': eight edits, the maximum on a substitution
    start = [0] * 9 + [1] * 8
    orig = ["N"] * 5 + [""] * 4 + ["C"] * 4 + [""] * 4
    mut = ["", "A", "C", "G", "T", "A", "C", "G", "T"] + ["", "A", "G", "T", "A", "C", "G", "T"]
    score = [2.0, -1.0, -1.0, 0.0, -1.0, -3.0, 2.0, -1.0, 1.0] + [-5.0, -4.0, -1.0, -2.0, -3.0, -3.0, -3.0, -3.0]
    table, margin, slot, npos = point_table_from_list(2, start, orig, mut, score)
    assert not np.isnan(table[0]).any() and np.array_equal(np.isnan(table[1]), np.arange(9) == 2)
    assert margin.tolist() == [2.0, -1.0] and slot.tolist() == [0, 3] and npos.tolist() == [3, 0]


def test_phred_from_margin_hand_values():
    ln10 = np.log(10.0)
    q = phred_from_margin([0.0, 3.5, -1e-6, -ln10, -2 * ln10, -1000.0, -0.25 * ln10 * (1 + 1e-9), -0.25 * ln10 * (1 - 1e-9)], 12)
    assert q.dtype == np.uint8 and q.shape == (12,)
    #                     >= 0  >= 0  ~0  10  20  capped  2.5 and a bit: 3; a bit less: 2; four positions without a row
    assert q.tolist() == [0, 0, 0, 10, 20, 93, 3, 2, 0, 0, 0, 0]
    assert phred_from_margin([-np.inf, -9.4 * ln10], 6).tolist() == [93, 93, 0, 0, 0, 0]
    assert phred_from_margin(np.zeros(0), 3).tolist() == [0, 0, 0]


def test_write_fastq_text():
    out = io.StringIO()
    write_fastq(out, "region_1", "ACGT", np.array([0, 10, 40, 93], dtype=np.uint8))
    assert out.getvalue() == "@region_1\nACGT\n+\n!+I~\n"
    with pytest.raises(ValueError):
        write_fastq(out, "x", "ACGT", [1, 2])


def test_variant_points_text_equals_variant_region():
    P = dict(P0, end_trim=20.0)
    draft, events, truth = synth.make_region(300, 5, 72, B.oracle_swalign, P)
    draft = draft[:150] + "N" + draft[151:]          # a position with nine edits
    want = io.StringIO()
    ms = variant_region(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P), [], region_start=100, out=want)
    got = io.StringIO()
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P)
    tables, percent = variant_points([pa], region_starts=[100], out=got)
    assert got.getvalue() == want.getvalue() and got.getvalue().startswith("100\t")
    assert len(tables) == 1 and tables[0][0].shape == (len(draft) - 4, 9)
    # Variant.py:80-93 on the MutationScore list
    trim = P["end_trim"]
    inside = [m for m in ms if m.start - 100 > trim and m.start - 100 < len(draft) - trim]
    assert inside and percent == [100 * float(sum(m.score > 0 for m in inside)) / len(inside)]
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))
    # one PSAlign instead of a list
    one = variant_points(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P), region_starts=100)
    assert np.array_equal(one[0][0][0], tables[0][0], equal_nan=True) and one[1] == percent


def test_consensus_region_qualities_change_nothing_else():
    P = dict(P0, end_trim=20.0)
    draft, events, truth = synth.make_region(300, 6, 75, B.oracle_swalign, P)
    runs = []
    for q in (None, []):
        B.reset_rand()
        pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P)
        log = []
        res = consensus_region(pa, P, refseq=truth, log=log, qualities=q)
        runs.append((res, log, [ev.ref_align.copy() for ev in pa.events], [ev.ref_like.copy() for ev in pa.events], q))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert all(np.array_equal(x, y) for x, y in zip(a[2] + a[3], b[2] + b[3]))
    q = b[4]
    assert len(q) == 1 and q[0].dtype == np.uint8 and len(q[0]) == len(b[0][0]) < len(draft)
    # the qualities are those of the untrimmed sequence's table, cut like the sequence
    full = b[1][-1][2]
    assert b[0][0] == full[20:-20]
    pa = B.make_pa(B.OraclePSAlign, full, [copy.deepcopy(ev) for ev in events], P)
    for ev, ra, rl in zip(pa.events, b[2], b[3]):
        ev.ref_align[:], ev.ref_like[:] = ra, rl
    assert np.array_equal(q[0], phred_from_margin(pa.PointTable(table=False)[1], len(full))[20:-20])
    assert q[0].max() > 0
    # fewer than 5 events: handed back untouched, no qualities
    q = []
    assert consensus_region(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events[:4]), P), P, qualities=q) == (draft, 100) and q == [None]


def test_new_symbols_are_optional_and_the_checkers_still_load():
    for name in NEW:
        assert name in _capi.SYMBOLS and name in _capi.OPTIONAL
    api = B.oracle_api()
    assert set(NEW) <= api.missing and api.missing <= _capi.OPTIONAL
    with pytest.raises(_capi.PoreseqError):
        api.batch_point_table([], [])
