"""`poreseq variant -v` on the GPU: `ps_score_sequences` (the map build of the Smith-Waterman traceback, k_remap, one chain of
(sequence x event) alignments) against the reference's own loop run on the reference build (tests/golden/variant_seqs.json), the
oracle's literal loop of Copy / RealignTo / ScoreEvents and the HIP library's own literal loop; under every forced kernel form and
band mode; on resident handles of several regions; in several chunks.  Tolerance 0 everywhere."""
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import variant_cases as VC
from poreseq_amd import _capi, consensus, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
GOLD, check_against_fixture = VC.GOLD, VC.check_against_fixture
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = VC.case(name, B.oracle_swalign)
    draft, events, p, vs = _CASES[name]
    return draft, copy.deepcopy(events), dict(p), list(vs)


class _env:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


def _literal_loop(pa, seqs):
    """Variant.py:52-59 through existing entry points only"""
    rows = []
    for s in seqs:
        pav = pa.Copy()
        pav.RealignTo(s)
        rows.append(pav.ScoreEvents())
    return rows


@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_batched_call_equals_the_reference_run(name):
    draft, events, p, vs = _case(name)
    assert VC.inputs_digest(draft, events, vs) == GOLD[name]["inputs"]
    pa = B.make_pa(PSAlign, draft, events, p)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        rows = pa.ScoreSequences([s for _, s in vs])
        n_map, n_remap, n_lists = api.prof_get("sw_map")[1], api.prof_get("remap")[1], api.prof_get("sw_lists")[1]
    finally:
        api.prof_enable(0)
    assert n_map >= 1 and n_remap >= 1          # the map build of the traceback and the device re-mapping ran ...
    assert n_lists == 0                          # ... and no index list was built inside the call
    check_against_fixture(name, pa, vs, rows=rows)
    assert pa.sequence == draft


@pytest.mark.parametrize("name", ["L600", "L3000"])
def test_batched_call_equals_the_oracle_literal_loop(name):
    draft, events, p, vs = _case(name)
    seqs = [s for _, s in vs]
    want = _literal_loop(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), p), seqs)
    got = B.make_pa(PSAlign, draft, events, p).ScoreSequences(seqs)
    assert got.tolist() == want


def test_batched_call_equals_the_librarys_own_literal_loop_at_10_kb():
    draft, events, p, vs = _case("L10000")
    seqs = [s for _, s in vs]
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        want = _literal_loop(B.make_pa(PSAlign, draft, copy.deepcopy(events), p), seqs)
        assert api.prof_get("sw_lists")[1] == len(seqs) and api.prof_get("sw_map")[1] == 0    # (the counters tell the two paths apart)
    finally:
        api.prof_enable(0)
    got = B.make_pa(PSAlign, draft, events, p).ScoreSequences(seqs)
    assert got.tolist() == want


_FORCED = {
    "sweep_4x1": dict(form=(4, 1), sweep_min=0), "sweep_4x2": dict(form=(4, 2), sweep_min=0), "sweep_2x4": dict(form=(2, 4), sweep_min=0),
    "k_fill": dict(sweep_min=1 << 30), "band_off": dict(band="off"), "band_force": dict(band="force"),
}


@pytest.mark.parametrize("setting", sorted(_FORCED))
@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_results_do_not_depend_on_kernel_form_or_band_mode(name, setting):
    draft, events, p, vs = _case(name)
    cfg = _FORCED[setting]
    api = _capi.load_hip()
    pa = B.make_pa(PSAlign, draft, events, p)
    if "sweep_min" in cfg:
        api.set_sweep_min(cfg["sweep_min"])
    if "form" in cfg:
        api.set_sweep_form(*cfg["form"])
    try:
        with _env(PORESEQ_SW_BAND=cfg.get("band")):
            c0 = api.debug_sw_band()
            rows = pa.ScoreSequences([s for _, s in vs])
            c1 = api.debug_sw_band()
    finally:
        api.set_sweep_min(-1)
        api.set_sweep_form(0, 0)
    banded = c1["banded"] - c0["banded"]
    if setting == "band_off":
        assert banded == 0
    if setting == "band_force":
        assert banded == len({s for _, s in vs})       # every distinct pair went through the band fill (some fall back, certified or redone)
    for (vid, _), row in zip(vs, rows):
        assert row.tolist() == GOLD[name]["variants"][vid]["scores"], (setting, vid)


def test_the_align_data_is_left_as_it_was():
    draft, events, p, vs = _case("L600")
    api = _capi.load_hip()
    h = api.align_create(draft, events, p)
    try:
        def refs():
            out = []
            for e in range(len(events)):
                n = int(api.lib.ps_align_n_levels(h, e))
                ra, rl = np.empty(n), np.empty(n)
                api.check(api.lib.ps_align_get_event_refs(h, e, _capi._dp(ra), _capi._dp(rl)))
                out.append((ra, rl))
            return out
        base = api.score_alignments(h, len(events)).tolist()
        assert base == GOLD["L600"]["base"]
        before = refs()
        scores, acc = api.score_sequences(h, [s for _, s in vs], len(events))
        after = refs()
        for (a0, l0), (a1, l1) in zip(before, after):
            assert np.array_equal(a0, a1) and np.array_equal(l0, l1)
        assert api.align_sequence(h) == draft
        assert api.score_alignments(h, len(events)).tolist() == base
        for k, (vid, _) in enumerate(vs):
            assert scores[k].tolist() == GOLD["L600"]["variants"][vid]["scores"]
            assert acc[k] == GOLD["L600"]["variants"][vid]["accuracy"]
        # twice on the same handle: nothing was cached that changes the answer
        again, _ = api.score_sequences(h, [s for _, s in vs][::-1], len(events))
        assert np.array_equal(again[::-1], scores)
    finally:
        api.align_destroy(h)


def test_region_batch_on_resident_handles_equals_region_by_region():
    P = dict(VC.params("L3000"))
    cases = [_case("L600")[:3]]
    for seed in (5201, 5202):
        d, ev, _ = synth.make_region(300, 5, seed, B.oracle_swalign, P)
        cases.append((d, ev, P))
    rng = np.random.default_rng(5)
    seqs = [[s for _, s in _case("L600")[3]], [], [cases[2][0], synth.corrupt(rng, cases[2][0], 0.02, 0.02, 0.02), cases[2][0][10:250]]]
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(ev), p) for d, ev, p in cases]
    want = [pa.ScoreSequences(sv) for pa, sv in zip(pas, seqs)]
    orc = [B.make_pa(B.OraclePSAlign, d, copy.deepcopy(ev), p).ScoreSequences(sv) for (d, ev, p), sv in zip(cases, seqs)]
    api = _capi.load_hip()

    def refs(rb):
        out = []
        for i, pa in enumerate(pas):
            for e in range(len(pa.events)):
                n = int(api.lib.ps_align_n_levels(rb._h[i], e))
                ra, rl = np.empty(n), np.empty(n)
                api.check(api.lib.ps_align_get_event_refs(rb._h[i], e, _capi._dp(ra), _capi._dp(rl)))
                out += [ra, rl]
        return out

    with RegionBatch(pas) as rb:
        rb.load()
        before = refs(rb)
        got = rb.ScoreSequences(seqs)
        part = rb.ScoreSequences([seqs[2], seqs[0][:2]], idx=[2, 0])
        after = refs(rb)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))    # the resident AlignData are as they were
    assert len(got) == 3 and got[1].shape == (0, 5)
    for g, w, o in zip(got, want, orc):
        assert np.array_equal(g, w) and np.array_equal(g, o)
    assert np.array_equal(part[0], want[2]) and np.array_equal(part[1], want[0][:2])
    for pa, (d, ev, _) in zip(pas, cases):
        assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, ev))


def test_a_sequence_without_an_alignment_raises_and_is_named():
    draft, events, p, vs = _case("L600")
    pa = B.make_pa(PSAlign, draft, events, p)
    with pytest.raises(_capi.PoreseqError, match=r"sequence 2 has no alignment"):
        pa.ScoreSequences([draft, vs[2][1], ""])
    with pytest.raises(_capi.PoreseqError, match=r"sequence 1 has no alignment"):
        pa.ScoreSequences([draft, "N" * 50, vs[2][1]])                      # nothing scores above 0
    with RegionBatch([pa, B.make_pa(PSAlign, draft, copy.deepcopy(events), p)]) as rb:
        with pytest.raises(_capi.PoreseqError, match=r"sequence 0 of region 1 has no alignment"):
            rb.ScoreSequences([[draft], ["N" * 50]])
    assert pa.ScoreSequences([draft]).tolist() == [GOLD["L600"]["base"]]   # the library is usable after the error


_CHUNK_CHILD = r"""
import copy, json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import backends as B
import variant_cases as VC
from poreseq_amd import _capi
from poreseq_amd.poreseqcpp import PSAlign
draft, events, p, vs = VC.case("L10000", B.oracle_swalign)
seqs = VC.many_variants(draft, vs, %(n)d)
api = _capi.load_hip()
api.prof_enable(1)
api.prof_reset()
rows = B.make_pa(PSAlign, draft, events, p).ScoreSequences(seqs)
chunks = api.prof_get("variant_chunks")[1]
units = api.prof_units("variant_chunks")
sw = api.prof_get("sw_map")[1]
api.prof_enable(0)
print("RESULT " + json.dumps({"rows": rows.tolist(), "chunks": chunks, "units": units, "sw": sw, "info": api.info()}))
"""


def test_a_call_cut_into_several_chunks_gives_the_same_results():
    """48 sequences x 10 events of a 10 kb region take ~70 MB of step codes per sequence; under PORESEQ_DEVICE_FRACTION=0.02 the
    runtime's share is its 2 GB floor, so the call needs several alignment chunks.  Observed through the launch counters:
    "variant_chunks" counts the alignment chunks of the call (its units: the distinct sequences).  (The Smith-Waterman batch may
    still be one launch: most pairs run banded, ~3 MB of checkpoints each, against 250 MB per launch.)  A process of its own: the
    fraction is read once, before the first compute call."""
    n = 48
    code = _CHUNK_CHILD % {"root": B.ROOT, "tests": os.path.join(B.ROOT, "tests"), "n": n}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=dict(os.environ, PORESEQ_DEVICE_FRACTION="0.02"))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["chunks"] >= 2 and res["sw"] >= 1, res["info"]
    assert res["units"] == n - 1                                            # the duplicate is aligned and scored once
    draft, events, p, vs = _case("L10000")
    seqs = VC.many_variants(draft, vs, n)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        whole = B.make_pa(PSAlign, draft, events, p).ScoreSequences(seqs)
        assert api.prof_get("variant_chunks")[1] == 1                       # the whole device: one chunk
    finally:
        api.prof_enable(0)
    assert res["rows"] == whole.tolist()
    for k, (vid, _) in enumerate(vs):
        assert res["rows"][k] == GOLD["L10000"]["variants"][vid]["scores"], vid


def _recut_case():
    """one synthetic region of 900 bases with 8 events at the default realign_width, and four distinct candidate sequences: the
    draft, the truth, a copy with an SNV and a copy with a deletion and an insertion"""
    from poreseq_amd.util import DEFAULT_PARAMS
    p = dict(DEFAULT_PARAMS, verbose=0)
    draft, events, truth = synth.make_region(900, 8, 7500, B.oracle_swalign, p)
    snv = draft[:450] + ("A" if draft[450] != "A" else "C") + draft[451:]
    indel = draft[:300] + draft[302:600] + "G" + draft[600:]
    seqs = [draft, truth, snv, indel]
    assert len(set(seqs)) == 4
    return draft, events, p, seqs


_RECUT_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import backends as B
from test_hip_variant_seqs import _recut_case
from poreseq_amd.poreseqcpp import PSAlign
draft, events, p, seqs = _recut_case()
rows = B.make_pa(PSAlign, draft, events, p).ScoreSequences(seqs)
print("RESULT", rows.shape[0], rows.shape[1], rows.tobytes().hex())
"""
# PORESEQ_MAX_BATCH_GB at which the first chunk of _recut_case holds two sequences on the 64-slot guess and is cut again on the real
# width.  Without strip sweeps a chunk is sized by matrix_bytes(S, P, 1) = (S + 24) * P * 18 per job, S = levels + states + 1.  The
# region's events have 844 to 870 levels, 6866 in all, and a sequence of 898 to 900 bases has at most 896 states: at P = 64 one
# sequence's eight jobs take (6866 + 8 * (896 + 25)) * 64 * 18 = 16.4 MB.  A budget of 40 MB holds two of them (32.8 MB) and not three
# (49.2 MB).  realign_width 300 needs far more than 64 slots per anti-diagonal (guess_slots_w(300) = 384), and at any width above
# 64 slots — 128 or more — the two sequences' matrices take at least 65.6 MB, over 1.2 x 40 MB = 48 MB: the chunk is cut again, to
# one sequence per chunk.  (0.2, FindMutations' budget at this shape, would hold all four sequences: 65.6 MB; they are cut again only
# if the real width is 256 slots or more, 4 x 16.4 x 4 = 262 MB against 240 MB.)
RECUT_GB = "0.04"


def test_variant_chunks_are_cut_again_when_the_bands_are_wider_than_guessed():
    """ps_score_sequences sizes its chunks on a guess of the band footprint, through the chunk driver it shares with FindMutations
    (fwd_chunks); with a guess far too small (PORESEQ_DEBUG_GUESS_P) the first chunk must be cut again, and the scores stay the same
    bytes: those of the plain run and of the oracle's literal loop.  Two child processes, as the guess is read once."""
    code = _RECUT_CHILD % {"root": B.ROOT, "tests": os.path.join(B.ROOT, "tests")}

    def run(extra):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PORESEQ_TRACE="1", **extra))
        assert r.returncode == 0, r.stderr[-2000:]
        n, e, data = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0].split()[1:]
        return (int(n), int(e), bytes.fromhex(data)), r.stderr

    plain, err0 = run({})
    cut, err1 = run({"PORESEQ_DEBUG_GUESS_P": "64", "PORESEQ_NO_SWEEP": "1", "PORESEQ_MAX_BATCH_GB": RECUT_GB})
    print("\n".join(l for l in err1.splitlines() if "chunk" in l or "over the share" in l))
    assert "[ps] score_sequences:" in err0 and "variant chunk" not in err0 and "cut again" not in err0    # (traced, and nothing to report)
    assert "variant chunk" in err1 and "cut again" in err1
    assert cut == plain
    draft, events, p, seqs = _recut_case()
    want = np.array(_literal_loop(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), p), seqs), dtype=np.float64)
    assert plain == (len(seqs), len(events), want.tobytes())


def test_variant_sequences_prints_the_reference_lines():
    draft, events, p, vs = _case("L3000")
    pa = B.make_pa(PSAlign, draft, events, p)
    out = io.StringIO()
    got = consensus.variant_sequences(pa, dict(vs), out=out)
    want = GOLD["L3000"]["variants"]
    assert got == {vid: want[vid]["dscore"] for vid, _ in vs}
    assert out.getvalue() == "".join(want[vid]["line"] for vid, _ in vs)


def test_a_bad_offset_array_is_a_bad_argument():
    import ctypes as C
    draft, events, p, vs = _case("L600")
    api = _capi.load_hip()
    h = api.align_create(draft, events, p)
    try:
        scores, acc = np.zeros((2, len(events))), np.zeros(2)
        for off in ([0, 40, 30], [-1, 10, 20]):
            o = np.array(off, dtype=np.int64)
            rc = api.lib.ps_score_sequences(h, 2, o.ctypes.data_as(_capi.c_i64p), draft.encode("ascii"), _capi._dp(scores), _capi._dp(acc))
            assert rc == -1 and b"offset" in api.lib.ps_last_error()       # PS_ERR_BAD_ARG, nothing read through the offsets
    finally:
        api.align_destroy(h)
