"""Band mode of the Smith-Waterman fill (poreseq_amd/csrc/ps_sw.hip): a pair banded around the main diagonal either carries the
exactness certificate or is redone on the full matrix, so every result is bit-identical to the full fill and to the oracle.
PORESEQ_SW_BAND=force bands every pair, =off none; PORESEQ_SW_BAND_W sets the half-width.  The band counters (ps_debug_sw_band)
show which path ran.  The certificate itself is checked on the host in test_sw_band.py."""
import copy
import os

import numpy as np
import pytest

import backends as B
from poreseq_amd import _capi, synth
from poreseq_amd.poreseqcpp import PSAlign, swalign
from poreseq_amd.util import DEFAULT_PARAMS

pytestmark = pytest.mark.gpu
P0 = dict(DEFAULT_PARAMS, verbose=0)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


def _counters():
    return _capi.load_hip().debug_sw_band()


def _delta(c0, c1):
    return {k: c1[k] - c0[k] for k in c0}


def _pairs(rng):
    cases = []
    for n, err in [(3000, 0.005), (3000, 0.02), (5000, 0.01), (2000, 0.06), (4000, 0.12), (700, 0.03), (1, 0.0), (130, 0.0)]:
        s1 = synth.random_sequence(rng, n)
        cases.append((s1, synth.corrupt(rng, s1, err / 3, err / 3, err / 3) if n > 1 else s1))
    s1 = synth.random_sequence(rng, 2500)                        # length difference near 2 wb (wb = 128)
    cases.append((s1, s1[:40] + s1[290:]))
    cases.append((s1[250:], s1))
    unit = synth.random_sequence(rng, 37)                        # tandem repeat: ties everywhere, maxima off the diagonal
    cases.append((unit * 60, unit * 70))
    s1 = synth.random_sequence(rng, 3000)                        # an interspersed repeat placed off the diagonal
    rep = synth.random_sequence(rng, 400)
    cases.append((s1[:500] + rep + s1[500:], s1[:1500] + rep + s1[1500:]))
    s1 = synth.random_sequence(rng, 2200)                        # the best local alignment lies off the diagonal, near the band edge
    cases.append((synth.random_sequence(rng, 120) + s1, s1 + synth.random_sequence(rng, 120)))
    cases.append((synth.random_sequence(rng, 1500), synth.random_sequence(rng, 1600)))   # unrelated
    return cases


def test_swfull_band_force_equals_full_and_oracle():
    rng = np.random.default_rng(2024)
    cases = _pairs(rng)
    want = [B.oracle_swalign(a, b) for a, b in cases]
    res = {}
    for mode in ("off", "force"):
        with _env(PORESEQ_SW_BAND=mode, PORESEQ_SW_BAND_W="128"):
            c0 = _counters()
            res[mode] = [_capi.load_hip().swfull(a, b) for a, b in cases]
            d = _delta(c0, _counters())
        if mode == "off":
            assert d["banded"] == 0
        else:
            assert d["banded"] == len(cases)       # the band path ran
            assert d["fell_back"] >= 1             # and at least one pair failed its certificate
            assert d["edge"] >= 1                  # and one certified maximum lies within 64 of the band edge
            assert d["band_cells"] < d["full_cells"]
    for (sf, af, if1, if2), (sb, ab, ib1, ib2), w in zip(res["off"], res["force"], want):
        assert sf == sb
        assert (af == ab) or (np.isnan(af) and np.isnan(ab))
        assert np.array_equal(if1, ib1) and np.array_equal(if2, ib2)
        assert list(zip(ib1.tolist(), ib2.tolist())) == w[1]
        assert (ab == w[0]) or (np.isnan(ab) and np.isnan(w[0]))


def test_swfull_band_default_width_long_pairs():
    """the default half-width on long near-identical pairs (band mode chosen by auto) against the full fill and the oracle"""
    rng = np.random.default_rng(7)
    cases = []
    for n, err in [(10000, 0.01), (12084, 0.02), (9000, 0.1)]:
        s1 = synth.random_sequence(rng, n)
        cases.append((s1, synth.corrupt(rng, s1, err / 3, err / 3, err / 3)))
    for mode in ("off", "auto"):
        with _env(PORESEQ_SW_BAND=mode):
            c0 = _counters()
            got = [swalign(a, b) for a, b in cases]
            d = _delta(c0, _counters())
        if mode == "auto":
            assert d["banded"] == 2 and d["fell_back"] == 0   # the 90 % pair is not close enough to band
            auto = got
        else:
            off = got
    for (s1, s2), a, b in zip(cases, auto, off):
        assert a[1] == b[1]
        assert a[1] == B.oracle_swalign(s1, s2)[1]


def test_find_mutations_band_force_equals_off_and_oracle():
    draft, events, truth = synth.make_region(3000, 4, 777, B.oracle_swalign, P0)
    rng = np.random.default_rng(11)
    seeds = [synth.corrupt(rng, truth, e, e, e) for e in (0.002, 0.005, 0.01, 0.01, 0.02, 0.04)]
    seeds.append(truth[200:] + synth.random_sequence(rng, 150))
    res = []
    for cls, env in ((PSAlign, dict(PORESEQ_SW_BAND="off")), (PSAlign, dict(PORESEQ_SW_BAND="force", PORESEQ_SW_BAND_W="128")),
                     (B.OraclePSAlign, {})):
        with _env(**env):
            c0 = _counters() if cls is PSAlign else None
            pa = B.make_pa(cls, draft, copy.deepcopy(events), P0)
            nb = pa.Mutate(seqs=list(seeds), reps=2)
            if env.get("PORESEQ_SW_BAND") == "force":
                d = _delta(c0, _counters())
                assert d["banded"] >= len(seeds) and d["fell_back"] >= 1
        res.append((nb, pa.sequence, [ev.ref_align.copy() for ev in pa.events]))
    for r in res[1:]:
        assert r[0] == res[0][0] and r[1] == res[0][1]
        for x, y in zip(r[2], res[0][2]):
            assert np.array_equal(x, y)


# pairs at the edge of a band strip (512 columns) and of its row window: one column or row more or less than a strip, a strip's
# worth of columns against one row block, a single row against a second strip of one column
EDGE_LENGTHS = [(511, 513), (512, 512), (513, 511), (64, 512), (1, 513)]
_edge = {}


def _edge_cases():
    """the pairs and the oracle's index lists and the summaries read off them, computed once"""
    if not _edge:
        rng = np.random.default_rng(513)
        pairs = []
        for n1, n2 in EDGE_LENGTHS:
            base = synth.random_sequence(rng, max(n1, n2))
            s2 = list(base[:n2])
            for k in range(5, n2, 17):
                s2[k] = "ACGT"[int(rng.integers(0, 4))]
            pairs.append((base[:n1], "".join(s2)))
        lists = [B.oracle_api().swfull(a, b) for a, b in pairs]
        _edge.update(pairs=pairs, lists=lists, sums=[_capi.summary_from_lists(a, b, *w) for (a, b), w in zip(pairs, lists)])
    return _edge["pairs"], _edge["lists"], _edge["sums"]


@pytest.mark.parametrize("mode,width", [("force", "64"), ("force", "128"), ("off", "128")])
def test_strip_edge_pairs_lists_and_summaries(mode, width):
    """index lists (swfull) and summaries (one batch) of pairs whose lengths sit on a strip's edge, banded at two widths and on the
    full matrix, exactly the oracle's swfull and summary_from_lists of it (the layout these pairs stress: test_sw_layout.py)"""
    pairs, want_lists, want_sums = _edge_cases()
    hip = _capi.load_hip()
    with _env(PORESEQ_SW_BAND=mode, PORESEQ_SW_BAND_W=width):
        c0 = _counters()
        got_lists = [hip.swfull(a, b) for a, b in pairs]
        got_sums = hip.sw_summaries(pairs)
        d = _delta(c0, _counters())
    assert d["banded"] == (2 * len(pairs) if mode == "force" else 0)
    for n, g, w in zip(EDGE_LENGTHS, got_lists, want_lists):
        assert g[0] == w[0] and ((g[1] == w[1]) or (np.isnan(g[1]) and np.isnan(w[1]))), (n, g[:2], w[:2])
        assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), n
    for n, g, w in zip(EDGE_LENGTHS, got_sums, want_sums):
        assert tuple(g)[:-1] == tuple(w)[:-1] and ((g.accuracy == w.accuracy) or (np.isnan(g.accuracy) and np.isnan(w.accuracy))), (n, g, w)
