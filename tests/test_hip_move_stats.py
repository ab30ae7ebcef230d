"""The backtrace's moves on the GPU (k_move_stats; ps_move_stats / ps_batch_move_stats): `PSAlign.MoveStats` and
`RegionBatch.MoveStats` against util.moves_from_tables on the oracle's tables (move_cases.oracle_walk) — records, step codes and
columns equal, scores and the refs left in the handle those of ScoreEvents by bytes — on every case under every fill; the
invariants against ps_align_stats on the same handle; a ragged lock-step batch, a batch cut into sub-batches, poisoned scratch,
the launch counts, the keep_refs contract of a resident batch, and the C ABI's argument checks."""
import copy
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import backends as B
import move_cases as M
import poison_cases as PZ
from poreseq_amd import _capi
from poreseq_amd.batch import RegionBatch
from poreseq_amd.poreseqcpp import PSAlign

pytestmark = pytest.mark.gpu
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture
_HERE = os.path.dirname(os.path.abspath(__file__))


def launches(api):
    return api.prof_get("move_stats")[1]


def levels_of(events):
    return [ev.mean.size for ev in events]


def check_region(name, res, what):
    """one region's (scores, records, step, col) against the oracle's walk and its ScoreEvents"""
    scores, rec, step, col = res
    walk = M.oracle_walk(name) if name != M.NO_EVENTS else []
    M.check_records(rec, [w[0] for w in walk], what)
    assert M.same(step, [w[1] for w in walk]) and M.same(col, [w[2] for w in walk]), what
    if walk:
        assert scores.tobytes() == M.oracle_scored(name)[0].tobytes(), what
    else:
        assert scores.shape == (0,)


@pytest.mark.parametrize("name", M.NAMES)
@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
def test_every_case_under_every_fill(fwd_kernel, name):
    draft, events, par = M.case(name)
    api = _capi.load_hip()
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), par)
    api.prof_enable(1)
    api.prof_reset()
    try:
        res = api.move_stats(h, levels_of(events), True)
        n = launches(api)
        left = copy.deepcopy(events)
        api.align_update_events(h, left)
        _, stats = api.align_stats(h, E, False)
        plain = api.move_stats(h, levels_of(events))                            # without the per-level arrays: the same records
    finally:
        api.prof_enable(0)
        api.align_destroy(h)
    assert n == 1
    check_region(name, res, "%s, %s" % (name, fwd_kernel))
    _, ras, rls = M.oracle_scored(name)
    assert M.same([ev.ref_align for ev in left], ras) and M.same([ev.ref_like for ev in left], rls)
    for e in range(E):
        M.check_invariants(M.as_dict(res[1][e]), stats[e], "%s event %d" % (name, e))
    # (the second call realigned from the refs the first one left: where the alignment is a fixed point the records agree)
    assert plain[1].dtype == _capi.EVENT_MOVES and plain[1]["n_levels"].tolist() == levels_of(events)


def test_python_call_leaves_the_events_alone():
    draft, events, par = M.case("poor")
    pa = B.make_pa(PSAlign, draft, copy.deepcopy(events), par)
    res = pa.MoveStats(levels=True)
    check_region("poor", res, "PSAlign.MoveStats")
    s2, r2 = pa.MoveStats()
    assert s2.tobytes() == res[0].tobytes() and r2.tobytes() == res[1].tobytes()
    assert s2.tobytes() == np.asarray(pa.ScoreEvents(), dtype=np.float64).tobytes()
    assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, events))
    oracle = B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), par).MoveStats(levels=True)      # the fallback path: same bytes
    assert PZ.same_bytes(list(res), list(oracle))


@pytest.mark.parametrize("resident", [True, False])
def test_ragged_lock_step_batch(resident):
    pas = [B.make_pa(PSAlign, *M.case(n)) for n in M.BATCH]
    api = _capi.load_hip()
    rb = RegionBatch(pas, resident=resident)
    try:
        rb.load()
        api.prof_enable(1)
        api.prof_reset()
        try:
            res = rb.MoveStats(levels=True)
            n = launches(api)
        finally:
            api.prof_enable(0)
        back = rb.MoveStats(idx=[3, 1])
        rb.drop()
    finally:
        rb.close()
    assert n == 1                                                               # 3 + 3 + 0 + 3 events: one launch
    for name, r in zip(M.BATCH, res):
        check_region(name, r, "lock-step " + name)
        one = B.make_pa(PSAlign, *M.case(name)).MoveStats(levels=True)
        assert PZ.same_bytes(list(r), list(one))
    assert back[0][1].tobytes() == res[3][1].tobytes() and back[1][1].tobytes() == res[1][1].tobytes()
    assert back[0][0].tobytes() == res[3][0].tobytes() and back[1][0].tobytes() == res[1][0].tobytes()
    for pa, name in zip(pas, M.BATCH):
        assert all(np.array_equal(a.ref_align, b.ref_align, equal_nan=True) for a, b in zip(pa.events, M.case(name)[1]))


# The batch of test_ragged_lock_step_batch in a child process whose guess of the band footprint is far too small: a k_fill job at the
# guessed 64 slots takes (n0 + C + 1 + 24) * 64 * 18 bytes (matrix_bytes, ps_plan.h) — 1.8 + 3.0 + 0 + 1.8 MB for the four regions,
# under the budget of 7 MB, so the share does not cut the call — and several times that at its real footprint: realign answers
# "over the share: split" and the call is halved between AlignData until it fits.
SPLIT_GB = "0.007"
_CHILD = (
    "import pickle, sys\n"
    "sys.path[:0] = [%r, %r]\n"
    "import backends as B\n"
    "import move_cases as M\n"
    "from poreseq_amd import _capi\n"
    "from poreseq_amd.batch import RegionBatch\n"
    "from poreseq_amd.poreseqcpp import PSAlign\n"
    "api = _capi.load_hip()\n"
    "pas = [B.make_pa(PSAlign, *M.case(n)) for n in M.BATCH]\n"
    "api.prof_enable(1)\n"
    "api.prof_reset()\n"
    "with RegionBatch(pas, resident=False) as rb:\n"
    "    res = rb.MoveStats(levels=True)\n"
    "n = api.prof_get('move_stats')[1]\n"
    "api.prof_enable(0)\n"
    "pickle.dump((res, n), open(sys.argv[1], 'wb'))\n"
) % (os.path.dirname(_HERE), _HERE)


def test_batch_cut_into_sub_batches_gives_the_same_bytes(tmp_path):
    """One child process (PORESEQ_DEBUG_GUESS_P is read once per process)."""
    path = str(tmp_path / "cut.pkl")
    env = dict(os.environ, PORESEQ_TRACE="1", PORESEQ_DEBUG_GUESS_P="64", PORESEQ_NO_SWEEP="1", PORESEQ_MAX_BATCH_GB=SPLIT_GB)
    r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(path, "rb") as f:
        cut, n = pickle.load(f)
    print("\n".join(l for l in r.stderr.splitlines() if "over the share" in l))
    assert any(l.startswith("[ps] realign") and "over the share: split" in l for l in r.stderr.splitlines())
    assert n > 1                                                                # one launch per sub-batch
    for name, got in zip(M.BATCH, cut):
        check_region(name, got, "cut " + name)
        assert PZ.same_bytes(list(got), list(B.make_pa(PSAlign, *M.case(name)).MoveStats(levels=True)))


@pytest.mark.parametrize("pattern", PZ.PATTERN_IDS)
@pytest.mark.parametrize("fwd_kernel", ["sweep", "fill"], indirect=True)
def test_poisoned_scratch_changes_nothing(fwd_kernel, pattern):
    for name in ("untouched", "all_unaligned", "poor"):
        before = PZ.api(pattern).calls
        got = B.make_pa(PZ.CLASSES[pattern], *M.case(name)).MoveStats(levels=True)
        assert PZ.api(pattern).calls > before
        check_region(name, got, "poisoned (%s) %s" % (pattern, name))
    pas = [B.make_pa(PZ.CLASSES[pattern], *M.case(n)) for n in M.BATCH]
    with RegionBatch(pas, resident=False) as rb:
        res = rb.MoveStats(levels=True)
    for name, r in zip(M.BATCH, res):
        check_region(name, r, "poisoned (%s) lock-step %s" % (pattern, name))


@pytest.mark.parametrize("fwd_kernel", ["sweep", "fill"], indirect=True)
def test_launch_counts(fwd_kernel):
    """k_move_stats runs once per chain of a MoveStats call and in no other call"""
    api = _capi.load_hip()
    pas = [B.make_pa(PSAlign, *M.case(n)) for n in ("narrow", "wide")]
    api.prof_enable(1)
    api.prof_reset()
    try:
        counts = []
        for pa in pas:
            for call in (pa.ScoreEvents, pa.AlignStats, lambda: pa.AlignStats(realign=False), pa.MoveStats, lambda: pa.MoveStats(levels=True)):
                n0 = launches(api)
                call()
                counts.append(launches(api) - n0)
        with RegionBatch([B.make_pa(PSAlign, *M.case(n)) for n in ("narrow", "wide")]) as rb:
            for call in (rb.ScoreEvents, rb.AlignStats, rb.MoveStats, rb.Refine):
                n0 = launches(api)
                call()
                counts.append(launches(api) - n0)
    finally:
        api.prof_enable(0)
    assert counts == [0, 0, 0, 1, 1] * 2 + [0, 0, 1, 0]


def _state(pas):
    return [(pa.sequence, [(ev.ref_align.tobytes(), ev.ref_like.tobytes()) for ev in pa.events]) for pa in pas]


def test_resident_batch_keeps_its_refs_and_rebuilds_after_a_refit():
    names = ("wide", "narrow")
    mk = lambda: [B.make_pa(PSAlign, *M.case(n)) for n in names]
    alone = mk()
    with RegionBatch(alone) as rb:
        nb_alone = rb.Refine()
    pas = mk()
    with RegionBatch(pas) as rb:
        first = rb.MoveStats()
        again = rb.MoveStats(levels=True)
        nb = rb.Refine()
    assert nb == nb_alone and _state(pas) == _state(alone)                      # MoveStats left nothing behind in the handles
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(first, again))
    pas = mk()
    rb = RegionBatch(pas)
    try:
        rb.load()
        fits = rb.RefitTransitions(pool=False)
        scores = rb.ScoreEvents()
        rb.drop()
    finally:
        rb.close()
    for name, pa, fit, sc in zip(names, pas, fits, scores):
        want = B.make_pa(B.OraclePSAlign, *M.case(name))
        wfit = want.RefitTransitions()
        assert fit.params == wfit.params and fit.flags == wfit.flags
        assert [vars(e.model)["prob_skip"] for e in pa.events] == [vars(e.model)["prob_skip"] for e in want.events]
        assert sc == want.ScoreEvents() and sc != B.make_pa(PSAlign, *M.case(name)).ScoreEvents()      # the handles carry the new rates


def test_bad_arguments_of_the_c_abi():
    api = _capi.load_hip()
    draft, events, par = M.case("narrow")
    E = len(events)
    h = api.align_create(draft, copy.deepcopy(events), par)
    h0 = api.align_create(draft, [], par)
    try:
        mv, sc = np.zeros(E, dtype=_capi.EVENT_MOVES), np.zeros(E)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null moves"):                            # PS_ERR_BAD_ARG
            api.check(api.lib.ps_move_stats(h, _capi._dp(sc), None, None, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null moves"):
            api.check(api.lib.ps_move_stats(h0, None, None, None, None))
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\)"):
            api.check(api.lib.ps_move_stats(None, None, vp(mv), None, None))
        steps = (_capi.c_u8p * E)()                                                                     # an array of null pointers
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*null per-level array of event 0"):
            api.check(api.lib.ps_move_stats(h, None, vp(mv), steps, None))
        api.prof_enable(1)
        api.prof_reset()
        try:
            api.check(api.lib.ps_move_stats(h0, None, vp(mv), None, None))      # no events: PS_OK, nothing launched
            assert launches(api) == 0 and api.prof_get("fill")[1] + api.prof_get("sweep")[1] == 0
            api.check(api.lib.ps_move_stats(h, None, vp(mv), None, None))       # scores and the per-level arrays may be NULL
            assert launches(api) == 1
        finally:
            api.prof_enable(0)
        M.check_records(mv, [w[0] for w in M.oracle_walk("narrow")], "scores NULL")
    finally:
        api.align_destroy(h)
        api.align_destroy(h0)
