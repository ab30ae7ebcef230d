"""Phase of het edits on the CPU checkers: the path of a library without ps_score_mutation_phase (PSAlign.ScoreMutationPhase /
RegionBatch.ScoreMutationPhase over util.phase_from_deltas) against the definition's plain loops (phase_cases), the diploid regions
of synth.make_diploid_region, util.call_phase on canned values, consensus.variant_support with and without phase=True, the
preconditions of every case the GPU tests compare (phase_cases.decided), and the symbols."""
import copy
import ctypes
import io
import os
import re

import numpy as np
import pytest

import backends as B
import phase_cases as PC
import support_cases as S
import tiled_cases as T
from poreseq_amd import _capi, batch, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import variant_support
from poreseq_amd.util import call_phase, phase_from_deltas, phase_scan
from test_genotypes import TSV2, VCF2, _canned
from test_support import EDITS, SEQ

NEW = ("ps_score_mutation_phase", "ps_batch_score_mutation_phase")
P0 = PC.P0


def opa(draft, events, par=P0):
    return B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par)


@pytest.mark.parametrize("case", ["M9_W8", "skipped_site", "every_site_alone", "M65_S1", "sets14_S8", "M0"])
def test_fallback_equals_the_loops(case):
    draft, events, par, sites, W, lim, S_ = PC.shapes()[case]
    want, scores = PC.want_of(("shape", case), draft, events, par, sites, W, lim, S_)
    assert "ps_score_mutation_phase" in B.oracle_api().missing
    pa = opa(draft, events, par)
    got = pa.ScoreMutationPhase(sites, window=W, min_link=lim, max_sets=S_)
    PC.check(got, want, scores, case, exact=True)
    assert got[1].shape == (len(sites), W) and got[3].shape == (len(events), S_) and len(got[5]) == len(sites)
    assert pa.sequence == draft and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, events))   # self is not modified


def test_every_case_of_the_gpu_tests_is_decided_on_the_cpu():
    """(b)'s precondition for every shape and both diploid regions: no vote with a term within 1e-6 of 0 or of min_link.  A seed
    that breaks this is found here, not on the GPU."""
    for name, c in PC.shapes().items():
        want, _ = PC.want_of(("shape", name), *c)
        print("%s: M %d, sets %d, smallest |vote| %.3g, smallest ||vote| - min_link| %.3g" % (name, want["M"], want["n_sets"], want["margin_zero"], want["margin_link"]))
        assert PC.decided(want), name
    for key, want, _ in PC.split_wants():
        assert PC.decided(want), key
    for name in PC.DIPLOID:
        assert PC.decided(PC.want_of(("diploid", name), *PC.diploid(name)[:2], P0, PC.diploid(name)[3], 2, 0.0, 4)[0]), name
    w = {n: PC.want_of(("shape", n), *PC.shapes()[n])[0] for n in ("skipped_site", "every_site_alone", "M257_W8", "M129_S8", "M63_S1", "sets14_S8")}
    # the cases still do what they are there for
    k = 6                                                                    # the skipped edit's place in its list
    assert w["skipped_site"]["nterm"][k] == 0 and w["skipped_site"]["nterm"][k + 1] == 0 and w["skipped_site"]["link"]["n_both"][k - 1, 1] > 0
    assert w["skipped_site"]["set_ld"][k - 1] + 2 == w["skipped_site"]["set_ld"][k + 1] and max(w["skipped_site"]["nterm"]) > 1
    assert w["every_site_alone"]["n_sets"] == 12 > w["every_site_alone"]["S"] and min(w["every_site_alone"]["nterm"][1:]) > 0
    nb = w["M257_W8"]["link"]["n_both"]
    assert nb[248, 7] > 0 and nb[255, 0] > 0 and not nb[249, 7] and not nb[255, 1:].any() and not nb[256].any()      # partners at 256, zeros behind the end
    assert w["sets14_S8"]["n_sets"] == 14 > 8 and w["M63_S1"]["n_sets"] == 1 and w["M129_S8"]["n_sets"] == 1                # more sets than are tagged
    for n in ("M63_S1", "M129_S8", "sets14_S8"):
        assert (w[n]["hap"]["n1"] > 0).any() and (w[n]["hap"]["n2"] > 0).any() and -1 in w[n]["hap_ld"] and 1 in w[n]["hap_ld"][1:]
    assert (w["sets14_S8"]["hap"]["n1"][:, 7] > 0).all() and w["M129_S8"]["hap"]["n1"].max() > 2                            # three terms in a lane's partial
    lens, tl = w["M257_W8"]["M"], w["skipped_site"]["M"]
    assert (lens, tl) == (257, 13)


@pytest.mark.parametrize("name", list(PC.DIPLOID))
def test_diploid_regions_are_phased(name):
    draft, events, ev_hap, edits, carrier = PC.diploid(name)
    L, E, seed, sites = PC.DIPLOID[name]
    assert len(draft) == L and len(events) == E and [m.start for m in edits] == list(sites) and carrier == [1, 0, 1, 0]
    assert all(draft[m.start] == m.orig and m.mut != m.orig and len(m.mut) == 1 for m in edits) and ev_hap == [e % 2 for e in range(E)]
    want, scores = PC.want_of(("diploid", name), draft, events, P0, edits, 2, 0.0, 4)
    got = opa(draft, events).ScoreMutationPhase(edits)                      # window 2, min_link 0, max_sets 4
    PC.check(got, want, scores, "diploid " + name, exact=True)
    _sc, link, phase, hap, n_sets, _scored = got
    assert n_sets == 1 and phase["set"].tolist() == [0, 0, 0, 0]            # all sites in one set
    assert phase["hap"].tolist() == [1, -1, 1, -1]                          # the draft alternates the copies
    assert (link["n_both"][:3, 0] == E).all()
    first = hap["lik1"][:, 0] > hap["lik2"][:, 0]                           # the first copy carries site 0's alt: hap B
    assert first.tolist() == [h == 1 for h in ev_hap] and (hap["lik1"][:, 0] != hap["lik2"][:, 0]).all()
    print("smallest |lik1 - lik2| of an event: %.1f" % np.abs(hap["lik1"][:, 0] - hap["lik2"][:, 0]).min())
    assert (hap["n1"][:, 0] == 2).all() and (hap["n2"][:, 0] == 2).all() and not hap["n1"][:, 1:].any()


def test_make_region_is_unchanged_by_the_diploid_generator():
    a = synth.make_region(200, 4, 7790, B.oracle_swalign, P0)
    synth.make_diploid_region(200, 4, 7790, B.oracle_swalign, (50, 100), P0)
    b = synth.make_region(200, 4, 7790, B.oracle_swalign, P0)
    assert a[0] == b[0] and a[2] == b[2] and all(np.array_equal(x.mean, y.mean) and np.array_equal(x.ref_align, y.ref_align) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("resident", [True, False])
def test_region_batch_over_oracle_regions_equals_the_loops(resident):
    names = ["M9_W8", "M65_S1", "M0", "skipped_site"]
    cs = [PC.shapes()[n] for n in names]
    pas = [opa(c[0], c[1], c[2]) for c in cs]
    with RegionBatch(pas, resident=resident) as rb:
        got = rb.ScoreMutationPhase([c[3] for c in cs], window=[c[4] for c in cs], min_link=[c[5] for c in cs], max_sets=[c[6] for c in cs])
        one = rb.ScoreMutationPhase([cs[3][3]], idx=[3], window=4, max_sets=4)
        for pa, c in zip(pas, cs):
            assert pa.sequence == c[0] and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, c[1]))
        if resident:
            rb.drop()       # (closing a resident batch writes the re-aligned events back: not this test's subject)
    for n, c, g in zip(names, cs, got):
        PC.check(g, *PC.want_of(("shape", n), *c), "batch " + n, exact=True)
    PC.check(one[0], *PC.want_of(("shape", "skipped_site"), *cs[3]), "batch idx=[3]", exact=True)


def test_definition_on_random_terms_and_its_argument_checks():
    rng = np.random.default_rng(7780)
    E, M = 7, 150
    d = rng.choice([-1.0, 1.0], size=(E, M)) * 10.0 ** rng.uniform(-3, 2, size=(E, M))
    spans, starts = np.tile([1, M + 5], (E, 1)), np.arange(M)
    spans[3] = (40, 90)
    link, phase, hap, n_sets = phase_from_deltas(d, spans, starts, 1000, 3, 0.0, 8)
    terms = (starts.tolist(), d.tolist(), [tuple(s) for s in spans.tolist()])
    want = PC.yardstick(terms, 1000, E, 3, 0.0, 8)
    assert PC.same_phase(link, want["link"]) and PC.same_phase(phase, want["phase"]) and PC.same_phase(hap, want["hap"]) and n_sets == want["n_sets"]
    assert PC.same_phase(phase_scan(link, 0.0)[0], PC.replay(link, 0.0))
    assert link["n_both"][50, 0] == E and link["n_both"][39, 2] == E and link["n_both"][38, 0] == E - 1 and link["n_both"][88, 1] == E - 1 and not link["n_both"][M - 1].any()
    # swapping the sign of one site's terms swaps cis and trans of its pairs
    f = d.copy()
    f[:, 60] = -f[:, 60]
    flip = phase_from_deltas(f, spans, starts, 1000, 3, 0.0, 8)[0]
    assert np.array_equal(flip["n_cis"][59, 0], link["n_trans"][59, 0]) and np.array_equal(flip["n_trans"][60], link["n_cis"][60])
    # window 1 is the first column; a huge min_link leaves every site alone
    assert PC.same_phase(phase_from_deltas(d, spans, starts, 1000, 1, 0.0, 8)[0][:, 0], link[:, 0])
    alone = phase_from_deltas(d, spans, starts, 1000, 3, 1e300, 8)
    assert alone[3] == M and alone[1]["set"].tolist() == list(range(M)) and (alone[1]["hap"] == 1).all() and not alone[2]["n2"].any()
    # no events: all-zero links, every site its own set, no rows
    none = phase_from_deltas(np.empty((0, 5)), np.empty((0, 2)), np.arange(5), 1000, 2, 0.0, 4)
    assert not none[0]["n_both"].any() and none[1]["set"].tolist() == [0, 1, 2, 3, 4] and none[2].shape == (0, 4) and none[3] == 5
    assert phase_from_deltas(np.empty((3, 0)), spans[:3], [], 1000, 2, 0.0, 4)[3] == 0
    for bad in (dict(window=0), dict(window=9), dict(max_sets=0), dict(max_sets=9), dict(min_link=-1.0), dict(min_link=np.nan), dict(min_link=np.inf)):
        kw = dict(dict(window=2, min_link=0.0, max_sets=4), **bad)
        with pytest.raises(ValueError):
            phase_from_deltas(d, spans, starts, 1000, **kw)
        with pytest.raises(ValueError):
            opa(*PC.region(120, 5, 7401)).ScoreMutationPhase([], **kw)


def test_call_phase_on_canned_values():
    ph = np.array([(0.0, 1, 0), (-3.0, -1, 0), (0.0, 1, 1), (2.0, 1, 2), (5.0, 1, 2), (-1.0, -1, 2), (0.0, 1, 3)], dtype=_capi.EDIT_PHASE)
    gts = ['0/1', '0/1', '0/1', '0/1', '1/1', '0/1', '0/1']
    assert call_phase(gts, ph) == (['1|0', '0|1', '0/1', '1|0', '1/1', '0|1', '0/1'], [0, 0, None, 3, None, 3, None])
    pos = [101, 205, 300, 410, 420, 433, 500]
    assert call_phase(gts, ph, pos)[1] == [101, 101, None, 410, None, 410, None]       # PS: the POS of the set's first site
    assert call_phase([], np.zeros(0, dtype=_capi.EDIT_PHASE)) == ([], [])
    with pytest.raises(ValueError):
        call_phase(gts[:3], ph)


@pytest.mark.parametrize("fmt,want", [("tsv", TSV2), ("vcf", VCF2)])
def test_without_phase_the_writers_are_byte_for_byte_what_they_were(monkeypatch, fmt, want):
    seen = _canned(monkeypatch)
    monkeypatch.setattr(batch.RegionBatch, "ScoreMutationPhase", lambda *a, **k: pytest.fail("phase=False makes no phase call"))
    muts = [S.edit(1000 + st, o, m) for st, o, m, _ in EDITS]
    out = io.StringIO()
    res = variant_support([opa(SEQ, [], T.P0)], [muts], region_starts=[1000], out=out, fmt=fmt, chrom="chr7", ploidy=2, sample="NA12878", phase=False)
    assert out.getvalue() == want and len(res[0]) == 5 and seen["genotypes"] == 1
    for kw in (dict(ploidy=None), dict(ploidy=1), dict(ploidy=3)):
        with pytest.raises(ValueError, match="phase=True needs ploidy=2"):
            variant_support([opa(SEQ, [], T.P0)], [muts], phase=True, **kw)


def test_variant_support_phases_the_diploid_regions():
    regs = [PC.diploid("400"), PC.diploid("260")]
    pas = [opa(r[0], r[1]) for r in regs]
    plain, out, tsv = io.StringIO(), io.StringIO(), io.StringIO()
    base = variant_support(pas, PC.variant_lists(), out=plain, **PC.VARIANT_KW)
    res = variant_support(pas, PC.variant_lists(), out=out, phase=True, **PC.VARIANT_KW)
    head = [l for l in out.getvalue().splitlines() if l.startswith("#")]
    assert head[:-2] + head[-1:] == [l for l in plain.getvalue().splitlines() if l.startswith("#")] and head[-2] == PC.VARIANT_PS_LINE
    body = "".join(l + "\n" for l in out.getvalue().splitlines() if not l.startswith("#"))
    assert body == PC.VARIANT_BODY
    # against the run without phase: the same records, the het ones phased, PS the POS of the set's first site
    old = [l for l in plain.getvalue().splitlines() if not l.startswith("#")]
    new = body.splitlines()
    assert ["\t".join(l.split("\t")[:8]) for l in new] == ["\t".join(l.split("\t")[:8]) for l in old]
    samples = [l.split("\t")[9].split(":") for l in new]
    assert [s[0] for s in samples] == ["0/0", "1|0", "0|1", "0/0", "1|0", "0|1"] * 2
    assert [s[3] for s in samples] == [".", "1061", "1061", ".", "1061", "1061", ".", "5041", "5041", ".", "5041", "5041"]
    assert [":".join(s[1:3]) for s in samples] == [l.split("\t")[9].split(":", 1)[1] for l in old]
    for k, (r, b, reg) in enumerate(zip(res, base, regs)):
        assert len(b) == 5 and len(r) == 7 and all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(r[:2] + r[3:5], b[:2] + b[3:5]))
        assert r[5].tolist() == [1 if h == 1 else 2 for h in reg[2]]                   # every event's haplotype: B carries site 0's alt
        pick, link, phase, hap, n_sets = r[6]
        assert pick == [1, 2, 4, 5] and n_sets == 1 and phase["hap"].tolist() == [1, -1, 1, -1] and link.shape == (4, 2) and hap.shape == (len(reg[1]), 4)
        assert [s.start for s in r[2]] == [m.start for m in PC.variant_lists()[k]]     # absolute outside
    variant_support(pas, PC.variant_lists(), out=tsv, phase=True, **dict(PC.VARIANT_KW, fmt="tsv"))
    rows = [l.split("\t") for l in tsv.getvalue().splitlines()]
    assert rows[0][-3:] == ["phase_set", "hap", "vote"] and [r[13] for r in rows[1:7]] == ["0/0", "1|0", "0|1", "0/0", "1|0", "0|1"]
    assert [r[-3:] for r in rows[1:4]] == [[".", ".", "."], ["1060", "1", "0.0"], ["1060", "-1", repr(float(res[0][6][2]["vote"][1]))]]
    # a GQ threshold nobody passes: nothing is phased, every PS is '.'
    none = io.StringIO()
    variant_support(pas, PC.variant_lists(), out=none, phase=True, min_gq=100, **PC.VARIANT_KW)
    assert [l.split("\t")[9] + ":." for l in old] == [l.split("\t")[9] for l in none.getvalue().splitlines() if not l.startswith("#")]
    for pa, reg in zip(pas, regs):
        assert pa.sequence == reg[0] and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, reg[1]))


def test_new_symbols_are_declared_optional_and_exported_by_the_product():
    hdr = open(os.path.join(B.ROOT, "include", "poreseq_hip.h")).read()
    declared = set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _capi.SYMBOLS and name in _capi.OPTIONAL
    api = B.oracle_api()                             # the checker lacks them and still loads
    assert set(NEW) <= api.missing and api.missing <= _capi.OPTIONAL
    lib = ctypes.CDLL(_capi.HIP_LIB)                 # the product exports them
    for name in NEW:
        assert hasattr(lib, name), name
    assert _capi.load_hip().missing == set()
    assert (_capi.EDIT_LINK.itemsize, _capi.EDIT_PHASE.itemsize, _capi.EVENT_HAP.itemsize) == (32, 16, 24)
