"""The yardstick of ps_align_stats (the alignment census and the sums of the scaling fit), shared by test_align_stats.py (the
fallback path on the CPU checkers) and test_hip_align_stats.py (k_align_stats on the GPU): the definition of include/poreseq_hip.h
restated as plain loops over Python floats (IEEE double, every operation rounded once), and the cases.

  kind of level i     aligned iff ra[i] > 0, inserted iff ra[i] < 0, unaligned otherwise (0, NaN); column c = int(min(ra[i], 2147483647.0))
  census              in level order with p = the column of the previous ALIGNED level and prev_rep: d = c - p; d == 0 -> n_extend if
                      prev_rep else n_stay; d == 1 -> n_step; d > 1 -> n_jump, n_gap_cols += d - 1; d < 0 -> n_back; prev_rep = (d == 0);
                      the first aligned level sets prev_rep = False; first_col / last_col its column and the last one's
  fit                 an aligned level with 1 <= c <= S and k = states[c - 1] >= 0: n_fit, w = 1.0 / (s_k * s_k), wm = w * m_k,
                      r = mean[i] - m_k; sw += w; swm += wm; swmm += wm * m_k; swr += w * r; swmr += wm * r; swrr += (w * r) * r;
                      any other aligned level: n_nostate
  order of the adds   partial t = 0.0 takes the qualifying levels t, t + 256, ... ascending; the 256 partials go into 0.0 for t = 0 .. 255

Ints are compared for equality, the six sums byte for byte.  The states come from the oracle's ps_seq_to_states (cpp/Sequence.h)."""
import copy
import struct

import numpy as np

import backends as B
from poreseq_amd import _capi, synth
from poreseq_amd.events import PSEvent
from poreseq_amd.util import DEFAULT_PARAMS

P0 = dict(DEFAULT_PARAMS, verbose=0)
INTS = ("n_levels", "n_aligned", "n_insert", "n_unaligned", "n_step", "n_stay", "n_extend", "n_jump", "n_back", "n_nostate", "n_fit",
        "first_col", "last_col", "reserved", "n_gap_cols")
SUMS = ("sw", "swm", "swmm", "swr", "swmr", "swrr")
TILE = 256


def states_of(seq):
    return [int(s) for s in B.oracle_api().seq_to_states(seq)]


def record(states, mean, ra, level_mean, level_stdv):
    """one event's record as a dict, by the definition"""
    S, n = len(states), len(ra)
    rec = dict.fromkeys(INTS, 0)
    rec["n_levels"] = n
    part = {k: [0.0] * TILE for k in SUMS}
    have_prev, p, prev_rep = False, 0, False
    for i in range(n):
        x = float(ra[i])
        if not x > 0:
            rec["n_insert" if x < 0 else "n_unaligned"] += 1
            continue
        rec["n_aligned"] += 1
        c = int(min(x, 2147483647.0))
        if not have_prev:
            rec["first_col"] = c
            prev_rep = False
        else:
            d = c - p
            if d == 0:
                rec["n_extend" if prev_rep else "n_stay"] += 1
            elif d == 1:
                rec["n_step"] += 1
            elif d > 1:
                rec["n_jump"] += 1
                rec["n_gap_cols"] += d - 1
            else:
                rec["n_back"] += 1
            prev_rep = d == 0
        have_prev, p = True, c
        rec["last_col"] = c
        k = states[c - 1] if 1 <= c <= S else -1
        if k < 0:
            rec["n_nostate"] += 1
            continue
        rec["n_fit"] += 1
        m, s = float(level_mean[k]), float(level_stdv[k])
        w = 1.0 / (s * s)
        wm = w * m
        r = float(mean[i]) - m
        t = i % TILE
        part["sw"][t] += w
        part["swm"][t] += wm
        part["swmm"][t] += wm * m
        part["swr"][t] += w * r
        part["swmr"][t] += wm * r
        part["swrr"][t] += (w * r) * r
    for k in SUMS:
        tot = 0.0
        for t in range(TILE):
            tot += part[k][t]
        rec[k] = tot
    return rec


def want(seq, events, refs=None):
    """the records of every event of a region; refs: the ref_align arrays to reduce instead of the events' own"""
    st = states_of(seq)
    return [record(st, ev.mean.tolist(), (ev.ref_align if refs is None else refs[e]).tolist(), ev.model.level_mean.tolist(),
                   ev.model.level_stdv.tolist()) for e, ev in enumerate(events)]


def check(got, wanted, what=""):
    """got: _capi.EVENT_STATS [E]; wanted: the list of dicts"""
    assert got.dtype == _capi.EVENT_STATS and got.shape == (len(wanted),), what
    for e, w in enumerate(wanted):
        for k in INTS:
            assert int(got[k][e]) == w[k], "%s event %d %s: %d, want %d" % (what, e, k, int(got[k][e]), w[k])
        for k in SUMS:
            assert struct.pack("<d", float(got[k][e])) == struct.pack("<d", w[k]), \
                "%s event %d %s: %r, want %r" % (what, e, k, float(got[k][e]), w[k])


# ---- crafted ref arrays -----------------------------------------------------------------------------------------------------------
MIXED16 = [0, 0, 3, 3, 3, 3, -1, 3, 4, 6, -1, -1, 9, 8, 8, 0]
_MADE = {}


def _event(rng, ra):
    ra = np.array(ra, dtype=np.float64)
    return PSEvent(rng.normal(65.0, 12.0, ra.size), np.ones(ra.size), ra, np.zeros(ra.size), sequence="", model=synth.make_model(rng, False))


def _tiled(n, S):
    """n levels that step through the S columns, with a run of repeats and then a run of -1 straddling every multiple of 256 (for an
    n below 257: the last levels), a 0 and a NaN in between"""
    ra = [float(1 + (i * (S - 1)) // max(n - 1, 1)) for i in range(n)]
    for m in list(range(TILE, n + 1, TILE)) or [n - 8]:
        for i in range(m - 9, m - 3):                    # repeats of the column in front of them, up to the boundary ...
            if 0 < i < n:
                ra[i] = ra[m - 10]
        for i in range(m - 3, m + 4):                    # ... -1 across it ...
            if 0 <= i < n:
                ra[i] = -1.0
        for i in range(m + 4, m + 8):                    # ... and the same column again behind them
            if i < n:
                ra[i] = ra[m - 10]
    if n > 40:
        ra[20], ra[33] = 0.0, float("nan")
    return ra


def crafted():
    """name -> (sequence, events): the smallest shapes at which k_align_stats can go wrong; every event carries hand-written ref_align
    and is measured with realign=False"""
    if "crafted" in _MADE:
        return _MADE["crafted"]
    rng = np.random.default_rng(8801)
    seq = synth.random_sequence(rng, 64)
    S = 60
    carry = [float(1 + i // 8) for i in range(600)]
    carry[149] = 20.0
    for i in range(150, 450):
        carry[i] = -1.0                                   # 300 consecutive -1: the carry crosses a whole tile
    carry[450], carry[451] = 20.0, 20.0                   # a stay across them, then an extend
    past = [58.0, 59.0, 60.0, 61.0, 70.0, 1e12, float("inf"), 2147483647.0, 2147483648.0, 60.0, 0.5, 0.25, 1.0, 1.999]
    seq_n = seq[:30] + "N" + seq[31:]
    out = {
        "one_level": (seq, [_event(rng, [5]), _event(rng, [-1]), _event(rng, [0])]),
        "zeros_and_inserts": (seq, [_event(rng, [0] * 10), _event(rng, [-1] * 10)]),
        "mixed16": (seq, [_event(rng, MIXED16)]),
        "seven": (seq, [_event(rng, _tiled(n, S)) for n in (255, 256, 257, 513)] + [_event(rng, carry), _event(rng, past), _event(rng, [7])]),
        "past_S": (seq, [_event(rng, past)]),
        "non_acgt": (seq_n, [_event(rng, [float(c) for c in range(20, 40)]), _event(rng, _tiled(300, S))]),
        "no_events": (seq, []),
    }
    _MADE["crafted"] = out
    return out


BATCH = ("no_events", "mixed16", "seven")      # 0, 1 and 7 events


def pa_of(cls, seq, events, par=P0):
    return B.make_pa(cls, seq, copy.deepcopy(events), par)


# ---- recovery of a known distortion ---------------------------------------------------------------------------------------------------
DISTORTIONS = ((1.05, -1.5), (0.93, 2.0), (1.0, 0.0))
RECOVERY = (450, 6, 8811)      # bases, reads, seed: every read has more than 300 fitted levels (asserted)


def recovery_region(a, b):
    """(sequence, events): reads simulated on the sequence itself, their TRUE alignment as ref_align (synth.make_region without a
    draft error), read 0's model replaced by (level_mean - b) / a — so that level_mean * a + b is the model its levels were drawn from"""
    key = ("recovery", a, b)
    if key not in _MADE:
        L, E, seed = RECOVERY
        seq, events, truth = synth.make_region(L, E, seed, B.oracle_swalign, P0, draft_error=0)
        assert seq == truth
        events = copy.deepcopy(events)
        events[0].model.level_mean = (events[0].model.level_mean - b) / a
        _MADE[key] = (seq, events)
    return _MADE[key]


def check_recovery(stats, fits, a, b):
    """the fit of read 0 from `stats` against the exact-WLS bounds under the simulator's Gaussian level noise: with the fitted var,
    se(da) = var sqrt(sw / det), se(db) = var sqrt(swmm / det); |scale - a| <= 6 se(da), |shift - b| <= 6 se(db),
    |var - 1| <= 6 / sqrt(2 n_fit).  Every other read (undistorted) is held to the same bounds around (1, 0)."""
    for e, f in enumerate(fits):
        ta, tb = (a, b) if e == 0 else (1.0, 0.0)
        sw, swm, swmm, n_fit = float(stats["sw"][e]), float(stats["swm"][e]), float(stats["swmm"][e]), int(stats["n_fit"][e])
        assert n_fit >= 300 and f.ok, (e, n_fit, f)
        det = sw * swmm - swm * swm
        se_a, se_b = f.var * np.sqrt(sw / det), f.var * np.sqrt(swmm / det)
        print("read %d: scale %.5f (want %.2f, 6 se %.5f) shift %.4f (want %.2f, 6 se %.4f) var %.4f (bound %.4f)"
              % (e, f.scale, ta, 6 * se_a, f.shift, tb, 6 * se_b, f.var, 6 / np.sqrt(2 * n_fit)))
        assert abs(f.scale - ta) <= 6 * se_a and abs(f.shift - tb) <= 6 * se_b and abs(f.var - 1.0) <= 6 / np.sqrt(2 * n_fit), (e, f)
