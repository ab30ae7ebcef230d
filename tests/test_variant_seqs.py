"""`poreseq variant -v` (poreseq/Variant.py:42-63) on the CPU checkers: `consensus.variant_sequences` / `PSAlign.ScoreSequences`
against the reference's own statements run on the reference build (tests/golden/variant_seqs.json, made by
tests/golden/make_golden_variant_seqs.py), the ABI additions, and the re-mapping rule the HIP kernel compiles (ps_remap.h) against
`PSEvent.mapaligns`.  All comparisons are exact.  The HIP path itself is held to the same fixture in test_hip_variant_seqs.py."""
import copy
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import variant_cases as VC
from poreseq_amd import _capi, consensus, synth
from poreseq_amd.events import PSEvent

GOLD, check_against_fixture = VC.GOLD, VC.check_against_fixture
NEW = ("ps_score_sequences", "ps_batch_score_sequences")


@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_inputs_rebuild_to_the_stored_digest(name):
    draft, events, _, vs = VC.case(name, B.oracle_swalign)
    assert VC.inputs_digest(draft, events, vs) == GOLD[name]["inputs"]
    assert set(GOLD[name]["variants"]) == {vid for vid, _ in vs}
    assert dict(vs)["dup"] == dict(vs)["snv"]


@pytest.mark.parametrize("name", ["L600", "L3000"])
def test_variant_sequences_on_the_oracle_equals_the_reference(name):
    draft, events, p, vs = VC.case(name, B.oracle_swalign)
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), p)
    check_against_fixture(name, pa, vs)
    for vid, s in vs:
        assert B.oracle_swalign(draft, s)[0] == GOLD[name]["variants"][vid]["accuracy"]
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))


def test_variants_take_a_mapping_or_pairs_and_an_empty_alignment_raises():
    draft, events, p, vs = VC.case("L600", B.oracle_swalign)
    pa = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), p)
    a = consensus.variant_sequences(pa, vs[:3])
    assert consensus.variant_sequences(pa, dict(vs[:3])) == a
    assert consensus.variant_sequences(pa, iter(vs[:3])) == a
    assert pa.ScoreSequences([]).shape == (0, len(events))
    with pytest.raises(IndexError):                  # an empty alignment: the reference's IndexError on an empty pairs array
        pa.ScoreSequences([draft, ""])


def test_the_interpolation_quirk_is_in_the_fixture_cases():
    """A guard on the INPUTS, not on the feature (it needs nothing this module's subject adds): the fixture's `clip_ins` variant really is
    the hard case — clipped on the left and carrying an insertion, so levels left of the alignment land on numpy's line from (0, y0)"""
    draft, events, p, vs = VC.case("L600", B.oracle_swalign)
    pairs = np.array(B.oracle_swalign(draft, dict(vs)["clip_ins"])[1])
    lo = pairs[pairs[:, 0] > 0, 0].min()
    assert lo > 1 and (pairs[:, 0] == 0).any()
    hit = 0
    for ev in events:
        old = ev.ref_align.copy()
        new = copy.deepcopy(ev)
        new.mapaligns(pairs)
        hit += int(np.count_nonzero((old > 0) & (old < lo) & (new.ref_align > 0)))
    assert hit > 50


def test_new_symbols_are_declared_optional_and_exported_by_the_product():
    for name in NEW:
        assert name in _capi.SYMBOLS and name in _capi.OPTIONAL
    api = B.oracle_api()                             # the checker lacks them and still loads
    assert set(NEW) <= api.missing and api.missing <= _capi.OPTIONAL
    lib = ctypes.CDLL(_capi.HIP_LIB)                 # the product exports them
    for name in NEW:
        assert hasattr(lib, name), name
    assert _capi.load_hip().missing == set()


# ---- ps_remap.h against PSEvent.mapaligns --------------------------------------------------------------------------------------

def _expected(pairs, x):
    ev = PSEvent(np.zeros(len(x)), np.ones(len(x)), np.array(x, dtype=np.float64))
    ev.mapaligns(np.asarray(pairs))
    return ev.ref_align


def _remap_cases():
    cases = []
    # the Smith-Waterman lists of the fixture cases, on the events' own ref_align and on every index around the sequence
    for name in ("L600", "L3000"):
        draft, events, _, vs = VC.case(name, B.oracle_swalign)
        x = np.concatenate([ev.ref_align for ev in events] + [np.arange(-2, len(draft) + 4, dtype=np.float64)])
        for _, s in vs:
            cases.append((B.oracle_swalign(draft, s)[1], x))
    # random clipped pairs with insertions near the left end
    rng = np.random.default_rng(7)
    for _ in range(60):
        n = int(rng.integers(80, 400))
        s1 = synth.random_sequence(rng, n)
        a, b = int(rng.integers(1, n // 4)), int(rng.integers(3 * n // 4, n))
        at = a + int(rng.integers(8, 40))
        s2 = s1[a:at] + synth.random_sequence(rng, int(rng.integers(1, 9))) + s1[at:b]
        if rng.random() < 0.5:
            s2 = synth.corrupt(rng, s2, 0.02, 0.02, 0.02)
        pairs = B.oracle_swalign(s1, s2)[1]
        if pairs:
            cases.append((pairs, np.arange(-1, n + 3, dtype=np.float64)))
    # slopes that put slope * x + y0 on or beside .5 (1/6 at x = 3, 3/7, ...): lists with one inds1 == 0 entry in front of index lo
    for lo in range(2, 41):
        for d in range(-3, lo + 2):
            y0 = 11
            pairs = [(0, y0)] + [(lo + k, y0 + d + k) for k in range(6)]
            cases.append((pairs, np.concatenate([np.arange(0, lo + 8, dtype=np.float64), np.arange(0.25, lo + 6, 0.75)])))
            cases.append((pairs[1:3] + pairs[:1] + pairs[3:], np.arange(0, lo + 8, dtype=np.float64)))   # the entry behind lo: y0 all the same
    return cases


def test_remap_header_equals_mapaligns():
    cases = _remap_cases()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            for pairs, x in cases:
                want = _expected(pairs, x)
                f.write("%d %d\n" % (len(pairs), len(x)))
                f.write(" ".join(str(int(a)) for a, _ in pairs) + "\n")
                f.write(" ".join(str(int(b)) for _, b in pairs) + "\n")
                f.write(" ".join(float(v).hex() for v in x) + "\n")
                f.write(" ".join(float(v).hex() for v in want) + "\n")
        exe = os.path.join(tmp, "remap_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(B.ROOT, "tests", "native", "remap_check.cpp"), "-o", exe])
        res = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("mismatches=0"), out + res.stderr.decode()
    m = re.search(r"cases=(\d+) levels=(\d+) interpolated=(\d+)", out)
    assert m and int(m.group(1)) == len(cases) and int(m.group(3)) > 1000, out     # the interpolated branch is exercised
