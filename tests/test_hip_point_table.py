"""The per-position point-edit table on the GPU (k_point_table, ps_point_table / ps_batch_point_table): `PSAlign.PointTable`,
`RegionBatch.PointTable`, the consensus qualities and `variant_points` against the reference's vectors and the oracle's literal
construction (test_point_table.py).  Tolerance 0 throughout; NaN slots are compared as a mask."""
import copy
import ctypes
import io
import os
import threading

import numpy as np
import pytest

import backends as B
import golden_util as G
from point_cases import check_against_vector, oracle_table, same
from poreseq_amd import _capi, synth
from poreseq_amd.batch import RegionBatch
from poreseq_amd.consensus import consensus_region, consensus_regions, variant_points, variant_region
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS

pytestmark = pytest.mark.gpu
P0 = dict(DEFAULT_PARAMS, verbose=0)
SCORE_CASES = ["score_L300_E5", "score_L240_E4_narrow"]
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]      # conftest's fwd_kernel fixture: the four fill choices

_MADE = {}


def region(L, E, seed, params=P0):
    """(draft, events) of a synthetic region, made once"""
    key = (L, E, seed, tuple(sorted(params.items())))
    if key not in _MADE:
        draft, events, _ = synth.make_region(L, E, seed, B.oracle_swalign, params)
        _MADE[key] = (draft, events)
    return _MADE[key]


def hip_table(draft, events, params=P0, table=True):
    return B.make_pa(PSAlign, draft, copy.deepcopy(events), params).PointTable(table)


@pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)
@pytest.mark.parametrize("name", SCORE_CASES)
def test_fixtures_equal_the_reference_vector_under_every_fill(name, fwd_kernel):
    z = G.load(name)
    api = _capi.load_hip()
    api.prof_enable(1)
    api.prof_reset()
    try:
        pa = G.make(PSAlign, z)
        before = (pa.sequence, [ev.ref_align.copy() for ev in pa.events])
        got = pa.PointTable()
        ms, launches, nbytes = api.prof_get("point_table")
    finally:
        api.prof_enable(0)
    check_against_vector(z, got)
    assert same(got, G.make(B.OraclePSAlign, z).PointTable())
    n, E = len(pa.sequence) - 4, len(pa.events)
    assert launches >= 1 and nbytes == 8.0 * E * 8 * n + 88.0 * n
    assert pa.sequence == before[0] and all(np.array_equal(a.ref_align, b) for a, b in zip(pa.events, before[1]))   # self is not modified


@pytest.mark.parametrize("name", SCORE_CASES)
def test_without_the_table_the_records_are_the_same(name):
    z = G.load(name)
    full, lean = G.make(PSAlign, z).PointTable(), G.make(PSAlign, z).PointTable(table=False)
    assert lean[0] is None and same((None,) + full[1:], lean)
    # the table alone, through the C ABI
    api = _capi.load_hip()
    pa = G.make(PSAlign, z)
    with PSAlign._Data(pa, point_width=True) as d:
        n = len(pa.sequence) - 4
        tb = np.empty((n, 9))
        api.check(api.lib.ps_point_table(d.h, _capi._dp(tb), None, n))
    assert same((tb,) + full[1:], full)


def test_other_characters_have_nine_edits_and_invalid_states():
    draft, events = region(120, 4, 7301)
    draft = draft[:40] + "N" + draft[41:77] + "-" + draft[78:]
    got, want = hip_table(draft, events), oracle_table(draft, events, P0)
    assert same(got, want)
    assert not np.isnan(got[0][40]).any() and not np.isnan(got[0][77]).any() and np.isnan(got[0]).sum() == len(draft) - 4 - 2


def _variants():
    d7, e7 = region(700, 5, 7302)               # 696 positions: 25 blocks of 28, the last one partly filled
    d1, e1 = region(120, 5, 7303)
    inert = copy.deepcopy(e1)
    inert[2].ref_align[:] = 0                   # an event without alignment: its Alignment is a no-op (stripe_width 0)
    return {
        "700x5": (d7, e7, P0),
        "120x1": (d1, e1[:1], P0),
        "120x33": (d1, [copy.deepcopy(e1[k % 3]) for k in range(33)], P0),
        "inert_event": (d1, inert, P0),
        "point_width_0": (d1, e1, dict(P0, point_width=0.0)),
    }


@pytest.mark.parametrize("case", ["700x5", "120x1", "120x33", "inert_event", "point_width_0"])
def test_block_edges_and_the_event_sum_equal_the_oracle(case):
    draft, events, par = _variants()[case]
    assert same(hip_table(draft, events, par), oracle_table(draft, events, par))


RAGGED = [(300, 5, 7310), (240, 4, 7311), (500, 8, 7312)]


def _ragged_pas():
    return [B.make_pa(PSAlign, *map(copy.deepcopy, region(*r)), P0) for r in RAGGED]


@pytest.mark.parametrize("resident", [True, False])
def test_lock_step_equals_the_single_calls_and_leaves_the_regions_alone(resident):
    singles = [hip_table(*region(*r)) for r in RAGGED]
    pas = _ragged_pas()
    with RegionBatch(pas, resident=resident) as rb:
        got = rb.PointTable()
        lean = rb.PointTable([2, 0], table=False) if not resident else None   # (a subset, in another order, records only)
        nb = rb.Refine() if resident else None
    assert len(got) == 3 and all(same(g, s) for g, s in zip(got, singles))
    if not resident:
        assert same(lean[0], (None,) + singles[2][1:]) and same(lean[1], (None,) + singles[0][1:])
        for pa, r in zip(pas, RAGGED):
            d, ev = region(*r)
            assert pa.sequence == d
            assert all(np.array_equal(a.ref_align, b.ref_align) and np.array_equal(a.ref_like, b.ref_like) for a, b in zip(pa.events, ev))
        return
    # a Refine on the same resident batch afterwards: as on a batch that never ran PointTable
    fresh = _ragged_pas()
    with RegionBatch(fresh) as rb:
        want = rb.Refine()
    assert nb == want and [pa.sequence for pa in pas] == [pa.sequence for pa in fresh]


def test_resident_batch_keeps_sequences_and_python_events_until_it_is_closed():
    pas = _ragged_pas()
    rb = RegionBatch(pas).load()
    rb.PointTable()
    for pa, r in zip(pas, RAGGED):
        d, ev = region(*r)
        assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, ev))
    rb.drop()
    rb.close()


def test_dense_calls_queue_for_one_small_slab_and_match_alone():
    """tests/test_hip_variant.py's slab-pressure set-up (one slab of 0.3 GB in a subprocess, four threads of lock-step calls that wait for
    each other, a batch that is cut in halves, a region larger than the slab) with PointTable as the dense call"""
    import subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import copy, hashlib, sys, threading\n"
        "sys.path[:0] = [%r, %r]\n"
        "import numpy as np\n"
        "from poreseq_amd import synth, _capi\n"
        "from poreseq_amd.batch import RegionBatch\n"
        "from poreseq_amd.poreseqcpp import PSAlign, swalign\n"
        "from poreseq_amd.util import DEFAULT_PARAMS\n"
        "P = dict(DEFAULT_PARAMS, verbose=0)\n"
        "regs = [synth.make_region(700 + 150 * k, 6, 6100 + k, swalign, P) for k in range(8)]\n"
        "regs.append(synth.make_region(3000, 8, 6200, swalign, P))          # one region whose matrices alone exceed a 0.3 GB slab\n"
        "def mk(k):\n"
        "    pa = PSAlign(); pa.sequence, pa.events, pa.params = regs[k][0], copy.deepcopy(regs[k][1]), dict(P); return pa\n"
        "out = {}\n"
        "def work(t, ks):\n"
        "    with RegionBatch([mk(k) for k in ks]) as rb:\n"
        "        res = rb.PointTable()\n"
        "    out[t] = [hashlib.sha1(b''.join(np.ascontiguousarray(a).tobytes() for a in r)).hexdigest() for r in res]\n"
        "nth = int(sys.argv[1])\n"
        "groups = [[0, 1, 2], [3, 4], [5, 6, 7], [8]]\n"
        "if nth == 1:\n"
        "    for t, ks in enumerate(groups): work(t, ks)\n"
        "else:\n"
        "    th = [threading.Thread(target=work, args=(t, ks)) for t, ks in enumerate(groups)]\n"
        "    [x.start() for x in th]; [x.join() for x in th]\n"
        "print('DIGEST', hashlib.sha1(repr(sorted(out.items())).encode()).hexdigest())\n"
        "print('INFO', _capi.load_hip().info())\n"
    ) % (os.path.dirname(here), here)

    def run(nth, extra):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-c", code, str(nth)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        return [l for l in lines if l.startswith("DIGEST")][0], [l for l in lines if l.startswith("INFO")][0]

    want, _ = run(1, {})
    got, info = run(4, {"PORESEQ_SLABS": "1", "PORESEQ_SLAB_GB": "0.3"})
    assert got == want
    assert "1 of 1 allocated (0.3 GB" in info


def test_two_host_threads_equal_the_calls_alone():
    regs = [region(*r) for r in RAGGED[:2]]
    alone = [hip_table(d, e) for d, e in regs]
    got = [None, None]

    def work(k):
        for _ in range(3):
            got[k] = hip_table(*regs[k])

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert all(same(g, a) for g, a in zip(got, alone))


def test_consensus_regions_with_qualities_changes_nothing_else_and_equals_the_oracle():
    P = dict(P0, end_trim=20.0)
    made = [synth.make_region(L, E, seed, B.oracle_swalign, P) for L, E, seed in ((300, 6, 7320), (360, 4, 7321), (500, 7, 7322))]

    def lock_step(q):
        B.reset_rand()
        pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), P) for d, e, _ in made]
        logs, accs = [[] for _ in made], [[] for _ in made]
        res = consensus_regions(pas, P, refseqs=[t for _, _, t in made], logs=logs, accuracies=accs, qualities=q)
        refs = [[(ev.ref_align.copy(), ev.ref_like.copy()) for ev in pa.events] for pa in pas]
        return res, logs, accs, refs

    plain, q = lock_step(None), []
    with_q = lock_step(q)
    assert with_q[:3] == plain[:3]
    for ra, rb in zip(with_q[3], plain[3]):
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(ra, rb))
    # the oracle, region by region in a fresh process's random stream
    want, want_q, want_logs = [], [], []
    for d, e, t in made:
        B.reset_rand()
        log = []
        want.append(consensus_region(B.make_pa(B.OraclePSAlign, d, copy.deepcopy(e), P), P, refseq=t, log=log, qualities=want_q))
        want_logs.append(log)
    assert with_q[0] == want and with_q[1] == want_logs
    assert len(q) == 3 and q[1] is None and want_q[1] is None and with_q[0][1] == (made[1][2], 100)   # (handed back as loaded: the refseq it was given)
    for k in (0, 2):
        assert q[k].dtype == np.uint8 and len(q[k]) == len(with_q[0][k][0]) and np.array_equal(q[k], want_q[k])
        assert q[k].max() > 0


def test_variant_points_over_two_regions_writes_the_reference_lines():
    regs = [region(*r) for r in RAGGED[:2]]
    want = io.StringIO()
    for (d, e), start in zip(regs, (100, 9000)):
        variant_region(B.make_pa(PSAlign, d, copy.deepcopy(e), P0), [], region_start=start, out=want)
    got = io.StringIO()
    pas = [B.make_pa(PSAlign, d, copy.deepcopy(e), P0) for d, e in regs]
    tables, percent = variant_points(pas, region_starts=[100, 9000], out=got)
    assert got.getvalue() == want.getvalue()
    assert all(same(t, hip_table(d, e)) for t, (d, e) in zip(tables, regs)) and len(percent) == 2
    for pa, (d, e) in zip(pas, regs):
        assert pa.sequence == d and all(np.array_equal(a.ref_align, b.ref_align) for a, b in zip(pa.events, e))


def test_wrong_position_count_is_a_bad_argument():
    api = _capi.load_hip()
    draft, events = region(*RAGGED[1])
    h = api.align_create(draft, copy.deepcopy(events), P0)
    try:
        L = len(draft)
        with pytest.raises(_capi.PoreseqError, match=r"\(-1\).*n = %d,.* %d positions" % (L, L - 4)):   # PS_ERR_BAD_ARG, both numbers
            api.point_table(h, L)
        tb, best = api.point_table(h, L - 4)
        assert tb.shape == (L - 4, 9) and best.shape == (L - 4,)
    finally:
        api.align_destroy(h)
    # a sequence shorter than five bases: no positions, success
    h = api.align_create("ACGT", [], P0)
    try:
        tb, best = api.point_table(h, 0)
        assert tb.shape == (0, 9) and best.shape == (0,)
    finally:
        api.align_destroy(h)
    lib = ctypes.CDLL(_capi.HIP_LIB)
    assert hasattr(lib, "ps_point_table") and hasattr(lib, "ps_batch_point_table") and api.missing == set()
