"""The cases of ps_move_stats (the backtrace's moves, counted on the device), shared by test_move_stats.py (the restatement
util.moves_from_tables against the oracle and the live reference, on the CPU) and test_hip_move_stats.py (k_move_stats on the GPU
against that restatement).

Small regions only: the smallest shapes at which the kernel can go wrong.  Each family names the branch it is there for, and
test_move_stats.py asserts on the oracle that the branch is reached (REACH): a family that stops reaching it is to be changed, not
dropped.

  narrow / wide       about 260 bases at realign_width 3 and 300, reads with a hole and a forward jump in ref_align (the band resumes,
                      skip runs form) and, in `wide`, a read that never aligned
  untouched / empty_read / column0   ref_cases' reads of 0, 1, 2, 255, 256, 257 and 513 levels: the tile edges of the 256-thread pass
  all_unaligned       ref_cases: a read without an aligned level next to live reads (inert: stripe_width == 0)
  single              tiled_cases' partial-span tiling: bands pinned to the first / last rows
  stay_run            80 more levels on one column: one STAY, then an EXTEND run that crosses a wavefront edge
  poor                a read whose model is far off over a stretch of columns (IGNORE), with levels cut out (skip runs longer than
                      1) and levels of noise put in (INSERT); a read whose first levels are noise (the walk ends on a score <= 0)
  mean_nan            edge_cases: an AlignData marked non-finite"""
import copy

import numpy as np

import backends as B
import edge_cases
import ref_cases
import tiled_cases
from poreseq_amd import synth, util
from poreseq_amd.util import DEFAULT_PARAMS

P0 = dict(DEFAULT_PARAMS, verbose=0)
PER_LEVEL = ref_cases.PER_LEVEL
INTS = ("n_levels", "inert", "top_level", "top_col", "low_level", "low_col", "end_kind", "n_match", "n_ignore", "n_insert", "n_stay", "n_extend",
        "n_skip_runs", "max_skip", "n_skip_cols")
RECORDED = ("n_match", "n_ignore", "n_insert", "n_stay", "n_extend")
_made = {}


def _take(ev, idx):
    """the event with its levels re-indexed by `idx` (repeats put levels in, gaps cut them out), in place"""
    idx = np.asarray(idx, dtype=np.int64)
    for name in PER_LEVEL:
        if hasattr(ev, name):
            setattr(ev, name, np.array(np.asarray(getattr(ev, name))[idx], dtype=np.float64))
    ev.makecontiguous()
    return ev


def _punched(events, draft_len):
    """read 0 with a hole, read 1 with a forward jump of 40 columns over 30 levels (sweep_cases.punch, without its dice)"""
    ev = copy.deepcopy(events)
    ev[0].ref_align[40:90] = 0
    s = slice(100, 130)
    ev[1].ref_align[s] = np.minimum(ev[1].ref_align[s] + 40, draft_len - 5) * (ev[1].ref_align[s] > 0)
    return ev


def _banded(width, seed, never=False):
    P = dict(P0, realign_width=float(width))
    draft, events, _ = synth.make_region(260, 5, seed, B.oracle_swalign, P)
    events = _punched(events, len(draft))
    if never:
        events[4].ref_align[:] = 0
    return draft, events, P


def _stay_run():
    draft, events, _ = synth.make_region(260, 3, 8902, B.oracle_swalign, P0)
    ev = events[0]
    at = 100
    assert ev.ref_align[at] > 0
    _take(ev, list(range(at)) + [at] * 81 + list(range(at + 1, ev.mean.size)))
    rng = np.random.default_rng(8903)
    ev.mean[at:at + 81] += rng.normal(0.0, 0.05, 81)      # (the same level again and again, up to measurement noise)
    return draft, events, dict(P0)


def _poor():
    draft, events, _ = synth.make_region(260, 4, 8904, B.oracle_swalign, P0)
    rng = np.random.default_rng(8905)
    st = synth.states_of(draft)
    # read 0: the model rows of the states of columns 120 .. 127 moved far off: those columns' emissions are poor, and the path
    # crosses them without an emission (a longer stretch would end the local alignment instead)
    ev = events[0]
    ev.model = copy.deepcopy(ev.model)
    rows = sorted(set(int(s) for s in st[119:127]))
    ev.model.level_mean = np.array(ev.model.level_mean, dtype=np.float64)
    ev.model.level_mean[rows] += 40.0
    # read 1: three and five consecutive levels cut out (the path skips their columns), six levels of noise put in (inserted)
    ev = events[1]
    n = ev.mean.size
    _take(ev, list(range(60)) + list(range(63, 150)) + list(range(155, 200)) + [200] * 7 + list(range(201, n)))
    at = 60 + 87 + 45
    ev.mean[at + 1:at + 7] = rng.uniform(150.0, 160.0, 6)
    # read 2: the first 40 levels are noise: the local alignment starts behind them, the walk ends on a score <= 0
    ev = events[2]
    ev.mean[:40] = rng.uniform(150.0, 160.0, 40)
    return draft, events, dict(P0)


BUILDERS = {
    "narrow": lambda: _banded(3, 8900),
    "wide": lambda: _banded(300, 8901, never=True),
    "untouched": lambda: ref_cases.case("untouched"),
    "empty_read": lambda: ref_cases.case("empty_read"),
    "column0": lambda: ref_cases.case("column0"),
    "all_unaligned": lambda: ref_cases.case("all_unaligned"),
    "single": lambda: tiled_cases.crafted("single", "truncated"),
    "stay_run": _stay_run,
    "poor": _poor,
    "mean_nan": lambda: edge_cases.region("mean_nan"),
}
NAMES = tuple(BUILDERS)
NO_EVENTS = "no_events"
BATCH = ("empty_read", "untouched", NO_EVENTS, "all_unaligned")      # a 0-level read, 513 levels, no events at all, an inert read
LEVEL_COUNTS = (0, 1, 2, 255, 256, 257, 513)


def longest_run(step, codes):
    """the longest run of consecutive levels whose move code is one of `codes`"""
    best = run = 0
    for s in np.asarray(step).tolist():
        run = run + 1 if s in codes else 0
        best = max(best, run)
    return best


# what a family is there for: name -> predicate over the region's walks (oracle_walk: per event (record dict, step, col, ..)),
# asserted by test_move_stats.py
REACH = {
    "narrow": lambda w: all(x[0]["n_skip_runs"] > 0 for x in w) and w[0][0]["low_level"] > 1,
    "wide": lambda w: w[4][0]["inert"] == 1 and all(x[0]["max_skip"] >= 2 for x in w[:4]),
    "untouched": lambda w: [x[0]["n_levels"] for x in w] == [1, 256, 513] and w[0][0]["end_kind"] == 1 and w[0][0]["low_level"] == 0,
    "empty_read": lambda w: [x[0]["n_levels"] for x in w] == [0, 255, 257] and w[0][0]["inert"] == 1,
    "column0": lambda w: [x[0]["n_levels"] for x in w] == [2, 255, 257],
    "all_unaligned": lambda w: w[1][0]["inert"] == 1 and not w[0][0]["inert"] and not w[2][0]["inert"],
    "single": lambda w: all(x[0]["low_col"] > 1 for x in w) and w[3][0]["top_level"] == w[3][0]["n_levels"] and w[3][0]["top_col"] < 350,
    "stay_run": lambda w: ("4" + "5" * 70) in "".join(str(int(s)) for s in w[0][1]),      # in level order: the STAY, then the EXTENDs
    "poor": lambda w: (longest_run(w[0][1], (3,)) >= 5 and longest_run(w[1][1], (2,)) >= 5 and w[1][0]["max_skip"] >= 5
                       and w[2][0]["end_kind"] == 0 and w[2][0]["low_level"] > 40),
    "mean_nan": lambda w: w[0][0]["end_kind"] == 1 and w[0][0]["low_level"] > 1 and all(x[0]["end_kind"] == 0 for x in w[1:]),
}


def case(name):
    """(draft, events, params) of a case; the caller owns the copies"""
    if name == NO_EVENTS:
        return case("untouched")[0], [], dict(P0)
    if name not in _made:
        _made[name] = BUILDERS[name]()
    d, e, p = _made[name]
    return d, copy.deepcopy(e), dict(p)


def as_dict(rec):
    return {k: int(rec[k]) for k in INTS}


def oracle_walk(name, api=None):
    """per event (record dict, step, col, ref_align, ref_like): util.moves_from_tables on the debug_fill tables of `api` (the oracle
    by default; computed once per case and left unchanged), with the inert record for an event the reference does not walk"""
    key = ("walk", name, api is None)
    if key in _made:
        return _made[key]
    lib = B.oracle_api() if api is None else api
    draft, events, par = case(name)
    out = []
    for e, ev in enumerate(events):
        n = ev.mean.size
        with np.errstate(invalid="ignore"):
            walks = int(par["realign_width"]) != 0 and bool(np.any(ev.ref_align > 0))
        if not walks:
            rec = dict.fromkeys(INTS, 0)
            rec["n_levels"], rec["inert"] = n, 1
            out.append((rec, np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), ev.ref_align.copy(), ev.ref_like.copy()))
            continue
        rec, step, col, ra, rl = util.moves_from_tables(*ref_cases.fill_tables(lib, draft, events, par, e, 0))
        out.append((as_dict(rec), step, col, ra, rl))
    _made[key] = out
    return out


def scored(api, name):
    """(scores, [ref_align], [ref_like]) that score_alignments of `api` leaves in a fresh AlignData of the case"""
    draft, events, par = case(name)
    E = len(events)
    h = api.align_create(draft, events, par)
    try:
        scores = api.score_alignments(h, E)
        api.align_update_events(h, events)
    finally:
        api.align_destroy(h)
    return np.asarray(scores, dtype=np.float64), [ev.ref_align.copy() for ev in events], [ev.ref_like.copy() for ev in events]


def oracle_scored(name):
    key = ("scored", name)
    if key not in _made:
        _made[key] = scored(B.oracle_api(), name)
    return _made[key]


def same(a, b):
    """equal by bytes, array by array (NaN markers of a ref_align that no walk rewrote included)"""
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def check_invariants(rec, stats, what=""):
    """the invariants of include/poreseq_hip.h: rec a record dict, stats the ps_event_stats record (or dict) of the refs the same
    call left"""
    recorded = sum(rec[k] for k in RECORDED)
    if rec["inert"]:
        assert all(rec[k] == 0 for k in INTS if k not in ("n_levels", "inert")), (what, rec)
        return
    assert recorded == (rec["top_level"] - rec["low_level"] + 1 if rec["low_level"] else 0), (what, rec)
    assert rec["n_match"] + rec["n_ignore"] + rec["n_skip_cols"] == rec["top_col"] - rec["low_col"], (what, rec)
    assert rec["n_skip_runs"] <= rec["n_skip_cols"] and rec["max_skip"] <= rec["n_skip_cols"], (what, rec)
    assert (rec["max_skip"] > 0) == (rec["n_skip_runs"] > 0) == (rec["n_skip_cols"] > 0), (what, rec)
    assert rec["n_match"] + rec["n_stay"] + rec["n_extend"] == int(stats["n_aligned"]), (what, rec, stats)
    assert rec["n_ignore"] + rec["n_insert"] == int(stats["n_insert"]), (what, rec, stats)
    assert int(stats["n_levels"]) == rec["n_levels"], (what, rec)


def check_records(got, want, what=""):
    """got: _capi.EVENT_MOVES [E]; want: the list of record dicts"""
    assert got.shape == (len(want),), what
    for e, w in enumerate(want):
        for k in INTS:
            assert int(got[k][e]) == w[k], "%s event %d %s: %d, want %d" % (what, e, k, int(got[k][e]), w[k])
