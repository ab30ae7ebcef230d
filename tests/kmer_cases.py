"""The yardstick of ps_kmer_stats (per event group and 5-mer state the sums of a model re-estimation), shared by test_kmer_stats.py
(the fallback path on the CPU checkers) and test_hip_kmer_stats.py (k_kmer_stats on the GPU): the definition of include/poreseq_hip.h
restated as plain loops over np.float64 scalars (every operation rounded once), and the cases.

  which levels enter  ra[i] > 0, c = int(min(ra[i], 2147483647.0)) with 1 <= c <= S, k = states[c - 1] in 0 .. 1023 (ps_align_stats' n_fit)
  terms               z = (mean[i] - m_k) / s_k;  u = stdv[i] / mu_k;  p = lam_k / mu_k  with lam_k = sd_mean[k]^3 / sd_stdv[k]^2
                      n += 1; sz += z; szz += z * z; sp += p; spu += p * u; spv += p / u     into table[groups[e]][k]
  order of the adds   every sum of one (g, k) is serial from 0.0: the events of the group in event order, levels ascending

Counts are compared for equality, the five sums byte for byte (struct.pack).  The states come from the oracle's ps_seq_to_states.
The library forms lam_k with the C library's pow; every model of this module has sd_mean and sd_stdv on a grid of 1 / 256, where
cube and square are exact in double, so the yardstick's plain products are the same number whatever pow rounds like (`quantised`)."""
import copy
import struct

import numpy as np

import backends as B
import stats_cases as S
from poreseq_amd import _capi, synth
from poreseq_amd.events import PSEvent

P0 = S.P0
SUMS = ("sz", "szz", "sp", "spu", "spv")
T = _capi.KMER_TILE      # levels the kernel stages per step
NS = 1024
_MADE = {}


def states_of(seq):
    return S.states_of(seq)


def quantised(events):
    """a deep copy of the events whose models' sd_mean / sd_stdv lie on the grid of 1 / 256"""
    out = copy.deepcopy(events)
    for ev in out:
        for name in ("sd_mean", "sd_stdv"):
            q = np.round(np.asarray(getattr(ev.model, name), dtype=np.float64) * 256.0) / 256.0
            assert (q > 0).all()
            setattr(ev.model, name, q)
    return out


def table(states, events, refs, groups, G):
    """the table as a dict: "n" int64 [G, 1024] and the five sums float64 [G, 1024], by the definition"""
    S_ = len(states)
    n = np.zeros((G, NS), dtype=np.int64)
    sums = {k: [[np.float64(0.0)] * NS for _ in range(G)] for k in SUMS}
    with np.errstate(all="ignore"):
        for e, ev in enumerate(events):
            g = int(groups[e])
            md = ev.model
            ra = np.asarray(refs[e], dtype=np.float64)
            for i in range(ra.size):
                x = float(ra[i])
                if not x > 0:
                    continue
                c = int(min(x, 2147483647.0))
                k = states[c - 1] if 1 <= c <= S_ else -1
                if k < 0 or k >= NS:
                    continue
                m, s = np.float64(md.level_mean[k]), np.float64(md.level_stdv[k])
                mu, sg = np.float64(md.sd_mean[k]), np.float64(md.sd_stdv[k])
                lam = ((mu * mu) * mu) / (sg * sg)          # (exact products on the grid)
                z = (np.float64(ev.mean[i]) - m) / s
                u = np.float64(ev.stdv[i]) / mu
                p = lam / mu
                n[g, k] += 1
                sums["sz"][g][k] = sums["sz"][g][k] + z
                sums["szz"][g][k] = sums["szz"][g][k] + z * z
                sums["sp"][g][k] = sums["sp"][g][k] + p
                sums["spu"][g][k] = sums["spu"][g][k] + p * u
                sums["spv"][g][k] = sums["spv"][g][k] + p / u
    out = {"n": n}
    for k in SUMS:
        out[k] = np.array(sums[k], dtype=np.float64).reshape(G, NS)
    return out


def groups_of(events, groups=None, n_groups=None):
    """the default grouping restated: the strand, two groups"""
    if groups is None:
        return [1 if ev.model.complement else 0 for ev in events], (2 if n_groups is None else n_groups)
    return list(groups), (max(groups) + 1 if n_groups is None else n_groups)


def want(seq, events, groups=None, n_groups=None, refs=None):
    grp, G = groups_of(events, groups, n_groups)
    return table(states_of(seq), events, [ev.ref_align for ev in events] if refs is None else refs, grp, G)


def pack(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return struct.pack("<%dd" % a.size, *a.tolist())


def check(got, wanted, what=""):
    """got: _capi.KMER_STATS [G, 1024]; wanted: the dict of `table`"""
    assert got.dtype == _capi.KMER_STATS and got.shape == wanted["n"].shape, (what, got.shape, wanted["n"].shape)
    assert got.dtype.itemsize == 48
    bad = np.argwhere(got["n"] != wanted["n"])
    assert not bad.size, "%s n[%d][%d]: %d, want %d" % (what, bad[0][0], bad[0][1], got["n"][tuple(bad[0])], wanted["n"][tuple(bad[0])])
    for k in SUMS:
        if pack(got[k]) == pack(wanted[k]):
            continue
        for g in range(got.shape[0]):
            for q in range(NS):
                a, b = float(got[k][g, q]), float(wanted[k][g, q])
                assert struct.pack("<d", a) == struct.pack("<d", b), "%s %s[%d][%d]: %r, want %r" % (what, k, g, q, a, b)


# ---- crafted ref arrays -----------------------------------------------------------------------------------------------------------
def _model(rng, complement):
    m = synth.make_model(rng, complement)
    m.sd_mean = np.round(m.sd_mean * 256.0) / 256.0
    m.sd_stdv = np.round(m.sd_stdv * 256.0) / 256.0
    return m


def _event(rng, ra, complement=False):
    ra = np.array(ra, dtype=np.float64)
    return PSEvent(rng.normal(65.0, 12.0, ra.size), rng.uniform(0.4, 2.5, ra.size), ra, np.zeros(ra.size), sequence="", model=_model(rng, complement))


def _walk(n, S_):
    """n levels that step through the S_ columns"""
    return [float(1 + (i * (S_ - 1)) // max(n - 1, 1)) for i in range(n)]


NAN_AT, INF_AT = 7, 23      # the columns that carry the NaN / the +inf level mean of "nonfinite"


def crafted():
    """name -> (sequence, events, groups or None, n_groups or None): the smallest shapes at which k_kmer_stats can go wrong; every event
    carries hand-written ref_align and is measured with realign=False"""
    if "crafted" in _MADE:
        return _MADE["crafted"]
    rng = np.random.default_rng(9901)
    seq = synth.random_sequence(rng, 64)
    S_ = 60
    past = S.crafted()["past_S"][1][0].ref_align.tolist()
    seq_n = seq[:30] + "N" + seq[31:]
    seq300 = synth.random_sequence(rng, 300)
    edges = [_event(rng, _walk(n, S_), complement=bool(q % 2)) for q, n in enumerate((1, T - 1, T, T + 1, 2 * T + 1))]
    holes = _walk(T + 40, S_)
    for i in range(T - 6, T + 5):
        holes[i] = -1.0 if i % 2 else 0.0                  # inserted and unaligned levels across the tile edge
    bad = _event(rng, _walk(120, S_))
    bad.mean[[i for i, c in enumerate(bad.ref_align) if c == NAN_AT][0]] = np.nan
    bad.mean[[i for i, c in enumerate(bad.ref_align) if c == INF_AT][0]] = np.inf
    four = [_event(rng, _walk(200, S_), complement=bool(q % 2)) for q in range(4)]
    # two events of one group, three levels each on the column 9, then the same two in the other order
    a, b = _event(rng, [9, 9, 9, 10]), _event(rng, [9, 9, 9, 11])
    out = {
        "tile_edges": (seq, edges + [_event(rng, holes)], None, None),
        "all_A": ("A" * 40, [_event(rng, _walk(2 * T + 70, 36)), _event(rng, _walk(90, 36), True)], None, None),
        "all_T": ("T" * 40, [_event(rng, _walk(T + 3, 36)), _event(rng, _walk(33, 36))], [0, 0], 1),
        "distinct": (seq300, [_event(rng, [float(c) for c in range(1, 297)])], [0], 1),
        "past_S": (seq, [_event(rng, past), _event(rng, past, True)], None, None),
        "non_acgt": (seq_n, [_event(rng, [float(c) for c in range(20, 40)]), _event(rng, _walk(300, S_), True)], None, None),
        "four_bases": ("ACGT", [_event(rng, [1, 2, 0, -1, 1])], None, None),
        "zeros_and_inserts": (seq, [_event(rng, [0] * 10), _event(rng, [-1] * 10, True)], None, None),
        "nonfinite": (seq, [bad, _event(rng, _walk(100, S_))], [0, 1], 2),
        "one_group": (seq, copy.deepcopy(four), [0, 0, 0, 0], 1),
        "group_per_event": (seq, copy.deepcopy(four), [0, 1, 2, 3], 4),
        "empty_group": (seq, copy.deepcopy(four), [0, 2, 0, 2], 3),
        "order_ab": (seq, [a, b], [0, 0], 1),
        "order_ba": (seq, [copy.deepcopy(b), copy.deepcopy(a)], [0, 0], 1),
        "no_events": (seq, [], None, None),
        "seven": (seq, [_event(rng, _walk(n, S_), complement=bool(q % 3 == 1)) for q, n in enumerate((40, T + 1, 7, 300, 1, 64, 129))],
                  [0, 2, 1, 1, 0, 2, 2], 3),
        "one_event": (seq, [_event(rng, _walk(77, S_))], [0], 1),
    }
    _MADE["crafted"] = out
    return out


BATCH = ("no_events", "one_event", "seven")      # 0, 1 and 7 events; 2, 1 and 3 groups


def pa_of(cls, seq, events, par=P0):
    return B.make_pa(cls, seq, copy.deepcopy(events), par)


def _self_checks():
    """what the cases are for, asserted on the yardstick"""
    cs = crafted()
    w = want(*cs["all_A"])
    assert w["n"][0, 0] == 2 * T + 70 and w["n"][1, 0] == 90 and w["n"].sum() == 2 * T + 160
    w = want(*cs["all_T"])
    assert w["n"][0, NS - 1] == T + 36 and w["n"].sum() == T + 36
    w = want(*cs["distinct"])
    assert w["n"].sum() == 296 and (w["n"] > 0).sum() >= 200                               # as many distinct k-mers as 300 bases have
    w = want(*cs["four_bases"])
    assert not w["n"].any()
    w = want(*cs["zeros_and_inserts"])
    assert not w["n"].any()
    seq, events, grp, G = cs["nonfinite"]
    st = states_of(seq)
    w = want(seq, events, grp, G)
    kn, ki = st[NAN_AT - 1], st[INF_AT - 1]
    assert kn != ki and np.isnan(w["sz"][0, kn]) and np.isnan(w["szz"][0, kn]) and np.isposinf(w["sz"][0, ki]) and np.isposinf(w["szz"][0, ki])
    fin = np.ones((2, NS), dtype=bool)
    fin[0, kn] = fin[0, ki] = False
    for k in SUMS:
        assert np.isfinite(w[k][fin]).all() and np.isfinite(w[k][0, [kn, ki]]).all() == (k in ("sp", "spu", "spv"))
    w = want(*cs["empty_group"])
    assert not w["n"][1].any() and w["n"][0].any() and w["n"][2].any()
    ab, ba = want(*cs["order_ab"]), want(*cs["order_ba"])
    assert (ab["n"] == ba["n"]).all() and any(pack(ab[k]) != pack(ba[k]) for k in SUMS)      # the order of the events is in the bits
    seq, events = cs["non_acgt"][:2]
    assert min(states_of(seq)) < 0


_self_checks()


def nonfinite_cells():
    """(the two (group, k-mer) cells that hold the NaN and the +inf of "nonfinite")"""
    st = states_of(crafted()["nonfinite"][0])
    return (0, st[NAN_AT - 1]), (0, st[INF_AT - 1])


# ---- regions with true alignments ---------------------------------------------------------------------------------------------------
def true_region(L=450, E=6, seed=9911):
    """(sequence, events): reads simulated on the sequence itself with their TRUE alignment as ref_align, models on the grid"""
    key = ("true", L, E, seed)
    if key not in _MADE:
        seq, events, truth = synth.make_region(L, E, seed, B.oracle_swalign, P0, draft_error=0)
        assert seq == truth
        _MADE[key] = (seq, quantised(events))
    return _MADE[key]


def top_kmers(seq, count=20):
    """the `count` most frequent 5-mer states of the sequence (ties by state id)"""
    st = np.array([s for s in states_of(seq) if s >= 0])
    n = np.bincount(st, minlength=NS)
    return sorted(np.argsort(-n, kind="stable")[:count].tolist())
