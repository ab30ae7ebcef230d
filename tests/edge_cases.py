"""Regions whose VALUES leave what `synth.make_region` draws (level means about N(65, 12), deviations 0.3 .. 2, default transition
probabilities), shared by test_edge_values.py (preconditions, the host's range predicate, the oracle against the live reference)
and test_hip_edge_values.py (the HIP path against the oracle).  Every case is the base region with a few entries overwritten:

  tier A  finite data inside the range in which the host tabulates reciprocals (poreseq_amd/csrc/ps_sane.h)
  tier B  `corner_*`: the extreme tuples of that range, and the tuple that overflowed under the range the library had before
  tier C  finite data outside the range: the IEEE-division builds
  tier D  tables whose emissions are infinite or NaN: -infinity and NaN are marked — the DP and the edit scoring
          run on them, ViterbiMutate refuses them; a +infinity emission is refused by ps_align_create
  tier E  `vit_*`: finite, unmarked data (IEEE-division builds) that kills ViterbiMutate's max-plus vector.  On a three-event
          region (BASE3) the trimmed mean drops nothing, so a single level whose emission is -inf or below -1e300 for every state
          leaves its kept position with back-pointer -1 and score -1e300 in all 1024 states, and every later position with it; so
          does a run of levels whose sum passes -1e300.  The rule: the deterministic back-trace (nkeep == 0) is p[T - 1] = argmax of
          the final scores, p[i - 1] = bp[i][p[i]]; where some bp[i][p[i]], i >= 1, is -1 the call answers PS_ERR_BAD_ARG naming the
          entry point, the region of a lock-step call and the first dead kept position.  bp[0] is never followed.  The stochastic
          back-traces (nkeep > 0) are defined on such tables and run.  `vit_trimmed` is the control on the four-event base region:
          the one -inf per state is the dropped quarter and no position dies.

`synth.make_region`'s seeded streams are not touched.
"""
import copy
import os
import subprocess
import tempfile

import numpy as np

import backends as B
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS, MutationInfo

P0 = dict(DEFAULT_PARAMS, verbose=0)
BASE = (260, 4, 5150)          # make_region(L, events, seed)
BASE3 = (260, 3, 5150)         # three events: at most three levels on a position, so the trimmed mean drops none (tier E)
LO, HI = 2.0 ** -128, 2.0 ** 128            # ps_sane.h: divisors, magnitudes of non-zero means
LAM_LO, LAM_HI = 2.0 ** -200, 2.0 ** 200    # lambda = sd_mean^3 / sd_stdv^2

# name -> (level changes [(event, field, index or slice, value)], model changes [(event, field, index or slice, value)], params)
# A slice of a model table changes that many 5-mers; a level change one level (or a run) of one event.
_S7 = slice(None, None, 7)
CASES = {
    "base": ([], [], {}),
    # ---- tier A
    "spike": ([(1, "mean", 40, 1e4), (1, "mean", 41, -300.0), (2, "mean", 100, 1e12)], [], {}),
    "sd_small": ([(1, "stdv", 40, 1e-3), (1, "stdv", 41, 1e-9), (2, "stdv", 7, 1e-30)], [], {}),
    "sd_big": ([(1, "stdv", 40, 50.0), (1, "stdv", 41, 1e6), (2, "stdv", 7, 1e30)], [], {}),
    "model_flat": ([], [(1, "level_stdv", slice(None), 1e-3)], {}),
    "skip0": ([], [], {"skip_t": 0.0, "skip_c": 0.0}),
    "ins0": ([], [], {"insert_t": 0.0, "insert_c": 0.0, "stay_t": 0.0}),
    "off0": ([], [], {"lik_offset": 0.0}),
    "off_big": ([], [], {"lik_offset": 40.0}),
    # ---- tier B: the ends of the accepted range.  corner_hi: the largest e = (sd - sm) / sm, t = e e lambda and q = t / sd
    # (2^256, 2^712, 2^584); corner_lo: a2 of one unit in the last place at the smallest binade, the smallest lambda and level
    # stdv, tiny means of either sign; corner_mean: the largest |x - mu| over the smallest level stdv (d = 2^257, d d = 2^514)
    "corner_hi": ([(1, "stdv", 40, HI), (2, "stdv", 7, HI)], [(1, "sd_mean", _S7, LO), (1, "sd_stdv", _S7, 2.0 ** -292)], {}),
    "corner_lo": ([(1, "stdv", 40, LO), (2, "mean", 100, LO), (2, "mean", 101, -LO), (2, "mean", 102, 0.0)],
                  [(1, "sd_mean", _S7, LO * (1 + 2.0 ** -52)), (1, "sd_stdv", _S7, 2.0 ** -92), (2, "level_mean", slice(None, None, 11), -LO),
                   (2, "level_mean", slice(3, None, 11), 0.0)], {}),
    "corner_mean": ([(1, "mean", 40, HI), (2, "mean", 100, -HI)], [(1, "level_stdv", _S7, LO), (2, "level_mean", _S7, HI)], {}),
    # e = 1e155, e e = +inf: finite inputs, -inf emissions.  Inside the range the library had before, where the tabulated build gave NaN
    "corner_overflow": ([(1, "stdv", 40, 1e60)], [(1, "sd_mean", _S7, 1e-95)], {}),
    # ---- tier C
    "ieee_small": ([(1, "stdv", 40, 1e-120), (2, "stdv", 7, 1e-120), (1, "mean", 60, 1e120)], [], {}),
    "ieee_big": ([(1, "stdv", 40, 1e120), (2, "stdv", 7, 1e120), (1, "mean", 60, 1e120)], [], {}),
    "model_sdmean_big": ([], [(1, "sd_mean", _S7, 1e40)], {}),
    # ---- tier E, on BASE3: finite, unmarked levels that kill ViterbiMutate's max-plus vector.  With three
    # events the trimmed mean drops nothing, so one level whose emission is -inf (d d or e e overflows) or below -1e300 for every
    # state makes the kept position's row -inf or below -1e300; vit_accum keeps every row above -1e300 and lets the running score pass it
    "vit_mean_overflow": ([(1, "mean", 100, 1e160)], [], {}),
    "vit_stdv_overflow": ([(1, "stdv", 100, 1e160)], [], {}),
    "vit_below_big": ([(1, "mean", 100, 1e151)], [], {}),
    "vit_accum": ([(1, "mean", slice(100, 114), 1.5e150)], [], {}),
    # the control on the four-event BASE: the one -inf of each state is the lowest quarter, dropped; no row dies
    "vit_trimmed": ([(1, "mean", 100, 1e160)], [], {}),
    # ---- tier D, marked: emissions of -infinity or NaN.  The DP and the edit scoring run on them; ViterbiMutate refuses them
    "mean_nan": ([(1, "mean", 40, float("nan"))], [], {}),
    "mean_inf": ([(1, "mean", 40, float("inf")), (2, "stdv", 9, float("inf"))], [], {}),
    "sd_neg": ([(1, "stdv", 40, -1.0)], [], {}),
    "model_nan": ([], [(1, "level_mean", _S7, float("nan")), (2, "sd_mean", slice(3, None, 7), float("nan"))], {}),
    "model_sd_neg": ([], [(1, "level_stdv", _S7, -1.0), (2, "sd_stdv", _S7, float("inf"))], {}),     # log sg = NaN; lambda = 0, log lambda = -inf
    # ---- tier D, refused by ps_align_create: a +infinity emission (stdv == 0 mirrored, level_stdv == 0, lambda = +inf, lik_offset)
    "sd_zero": ([(1, "stdv", 40, 0.0), (2, "stdv", 0, 0.0), (2, "stdv", -1, 0.0)], [], {}),
    "sd_zero_run": ([(1, "stdv", slice(40, 70), 0.0)], [], {}),
    "model_sd_zero": ([], [(1, "level_stdv", _S7, 0.0)], {}),
    "lam_inf": ([], [(2, "sd_stdv", _S7, 0.0)], {}),
    "off_inf": ([], [], {"lik_offset": float("inf")}),
}
TIER_A = ("spike", "sd_small", "sd_big", "model_flat", "skip0", "ins0", "off0", "off_big")
TIER_B = ("corner_hi", "corner_lo", "corner_mean")
TIER_C = ("ieee_small", "ieee_big", "model_sdmean_big", "corner_overflow")     # model_sdmean_big: 1e40 > 2^128, moved out of tier A
TIER_D_MARKED = ("mean_nan", "mean_inf", "sd_neg", "model_nan", "model_sd_neg")
TIER_D_REFUSED = ("sd_zero", "sd_zero_run", "model_sd_zero", "lam_inf", "off_inf")
TIER_D = TIER_D_MARKED + TIER_D_REFUSED
TIER_E_DEAD = ("vit_mean_overflow", "vit_stdv_overflow", "vit_below_big", "vit_accum")
TIER_E = TIER_E_DEAD + ("vit_trimmed",)
ON_BASE3 = TIER_E_DEAD
# tier E: the first kept position all of whose states have back-pointer -1 (every later one has too), pinned by test_edge_values.py
VIT_FIRST_DEAD = {"vit_mean_overflow": 100, "vit_stdv_overflow": 100, "vit_below_big": 100, "vit_accum": 109}
UNREACHABLE = "no state is reachable at kept position %d "
FINITE = ("base",) + TIER_A + TIER_B + TIER_C + TIER_E
# what the message of a tier-D refusal names first
NAMED = {"mean_nan": "event 1, level 40:", "mean_inf": "event 1, level 40:", "sd_neg": "event 1, level 40:", "model_nan": "event 1, model row 0:",
         "model_sd_neg": "event 1, model row 0:", "sd_zero": "event 1, level 40:", "sd_zero_run": "event 1, level 40:",
         "model_sd_zero": "event 1, model row 0:", "lam_inf": "event 2, model row 0:", "off_inf": "lik_offset inf"}

_made = {}


def _base(name="base"):
    key = BASE3 if name in ON_BASE3 else BASE
    if key not in _made:
        draft, events, _ = synth.make_region(*key, B.oracle_swalign, P0)
        _made[key] = (draft, events)
    return _made[key]


def region(name):
    """(draft, events, params) of a case; the caller owns the copies"""
    levels, model, par = CASES[name]
    draft, events = _base(name)
    events = copy.deepcopy(events)
    params = dict(P0, **par)
    for e, field, at, value in levels:
        getattr(events[e], field)[at] = value
    for e, field, at, value in model:
        getattr(events[e].model, field)[at] = value
    if par:
        for ev in events:
            ev.setparams(params)
    return draft, events, params


def altered_events(name):
    """events with an overwritten level or model entry (every event for a case that only changes parameters: event 1 then stands for all)"""
    levels, model, _ = CASES[name]
    return sorted(set(e for e, *_ in levels) | set(e for e, *_ in model)) or [1]


def altered_levels(name):
    """(event, level index >= 0) of every overwritten level"""
    _, events = _base(name)
    out = []
    for e, _field, at, _v in CASES[name][0]:
        n = events[e].mean.size
        idx = range(*at.indices(n)) if isinstance(at, slice) else [at % n]
        out += [(e, int(i)) for i in idx]
    return sorted(set(out))


def edit(start, orig, mut):
    mi = MutationInfo()
    mi.start, mi.orig, mi.mut = int(start), orig, mut
    return mi


def edits(draft, events, name):
    """20 random point edits, then a deletion, a substitution and insertions of one to three bases on and next to the draft position
    every overwritten level is aligned to (at most the first four levels of a run), and the same at the middle of the region for the
    cases that overwrite no level"""
    n = len(draft)
    muts = synth.random_point_mutations(np.random.default_rng(4242), draft, 20)
    spots = []
    for e, i in altered_levels(name)[:8]:
        on = np.flatnonzero(events[e].ref_align[:i + 1] > 0)
        if on.size:
            spots.append(int(events[e].ref_align[on[-1]]) - 1)        # the level itself, or the nearest aligned level before it
    if not spots:
        spots = [n // 2]
    for p0 in sorted(set(spots))[:4]:
        for p in (p0 - 1, p0, p0 + 1):
            p = min(max(p, 0), n - 6)
            sub = "ACGT"[("ACGT".index(draft[p]) + 1) % 4]
            muts += [edit(p, draft[p], ""), edit(p, draft[p], sub), edit(p, "", "G"), edit(p, "", "TC"), edit(p, "", "ACA")]
    return muts


# ---- what ps_align_create decides, by the library's own predicate ---------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
_exe = {}


def _native_exe(name, flags=()):
    """tests/native/<name>.cpp, built once per session (both programs include poreseq_amd/csrc/ps_sane.h: the code ps_align.cpp compiles)"""
    if name not in _exe:
        if "dir" not in _exe:
            _exe["dir"] = tempfile.TemporaryDirectory()
        exe = os.path.join(_exe["dir"].name, name)
        subprocess.check_call(["g++", "-O2", *flags, os.path.join(HERE, "native", name + ".cpp"), "-o", exe])
        _exe[name] = exe
    return _exe[name]


def emission_check_exe():
    return _native_exe("emission_check", ("-mfma", "-ffp-contract=off"))


def host_verdict(events, params=P0):
    """what ps_align_create decides about these tables, through ps_sane.h (tests/native/sane_classify.cpp): ("refused", build),
    ("marked", build) or ("unmarked", build), where build is "fast" or "ieee" """
    lines = ["P %s" % float(params["lik_offset"]).hex()]
    for ev in events:
        lines += ["L %s %s" % (float(m).hex(), float(s).hex()) for m, s in zip(ev.mean, ev.stdv)]
        md = ev.model
        lines += ["M %s %s %s %s" % tuple(float(v).hex() for v in row) for row in zip(md.level_mean, md.level_stdv, md.sd_mean, md.sd_stdv)]
    out = subprocess.run([_native_exe("sane_classify")], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode().split()
    assert out[2] == "records=%d" % len(lines), out
    return out[0], out[1]


# ---- results -------------------------------------------------------------------------------------------------------------------
def scores(lst):
    return np.array([s.score for s in lst])


def refs(pa):
    return [ev.ref_align.copy() for ev in pa.events] + [ev.ref_like.copy() for ev in pa.events]


def call_set(cls, name, support=True, viterbi=True):
    """every public call of one backend on a case, each on a fresh object: a dict of plain results (support=False: without
    ScoreMutationSupport, whose per-event terms the reference build does not export; viterbi=False: without Mutate("viterbi"))"""
    draft, events, par = region(name)
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), par)
    muts = edits(draft, events, name)
    out = {"ScoreEvents": mk().ScoreEvents(), "ScorePoints": scores(mk().ScorePoints()), "ScoreMutations": scores(mk().ScoreMutations(muts))}
    pa = mk()
    out["Refine"] = (pa.Refine(), pa.sequence, refs(pa))
    pa = mk()
    out["Mutate"] = (pa.Mutate(seqs=[ev.sequence for ev in events[:3]], reps=2), pa.sequence, refs(pa))
    if viterbi:
        B.reset_rand()
        pa = mk()
        out["Viterbi"] = (pa.Mutate(seqs="viterbi"), pa.sequence, refs(pa))
    out["PointTable"] = mk().PointTable()
    if support:
        sc, sup, _ = mk().ScoreMutationSupport(muts)
        out["Support"] = (np.asarray(sc, dtype=np.float64), sup)
    return out


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x), np.signbit(y)) for x, y in zip(a, b))


def same_floats(a, b):
    """tolerance 0, NaN matched as a mask"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def differences(got, want, keys=None):
    """names of the calls whose results differ (empty: equal)"""
    bad = []
    for k in (keys or want):
        g, w = got[k], want[k]
        if k in ("ScoreEvents", "ScorePoints", "ScoreMutations"):
            ok = same_floats(g, w)
        elif k in ("Refine", "Mutate", "Viterbi"):
            ok = g[0] == w[0] and g[1] == w[1] and same_arrays(g[2], w[2])
        elif k == "PointTable":
            ok = same_floats(g[0], w[0]) and same_floats(g[1], w[1]) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(g[2:], w[2:]))
        else:
            ok = same_floats(g[0], w[0]) and same_floats(g[1]["sum"], w[1]["sum"]) and all(np.array_equal(g[1][f], w[1][f]) for f in ("cover", "pos", "neg"))
        if not ok:
            bad.append(k)
    return bad


_oracle = {}


def oracle_once(key, make):
    """an oracle result computed once per session and handed out unchanged (callers must not write into it)"""
    if key not in _oracle:
        _oracle[key] = make()
    return _oracle[key]


def oracle_calls(name):
    return oracle_once(("calls", name), lambda: call_set(B.OraclePSAlign, name))


def fill_tables(api, name, e, direction):
    draft, events, par = region(name)
    h = api.align_create(draft, events, par)
    try:
        return api.debug_fill(h, e, direction, events[e].mean.size, len(draft) - 4)
    finally:
        api.align_destroy(h)


def oracle_fill(name, e, direction):
    return oracle_once(("fill", name, e, direction), lambda: fill_tables(B.oracle_api(), name, e, direction))


# ---- ordinary data for the IEEE-division builds (PORESEQ_EXACT_DIV=1): the smallest shapes that reach each instance -------------
# name -> (L, events, seed, realign_width).  k_fill's launcher (launch_fill, ps_kernels.hip) picks the form from P, the widest
# anti-diagonal footprint of the batch's bands + 9 rounded up to 64 lanes: P <= 256 alone -> the compact layout (CMP), P <= 512 ->
# the plain 512-thread form, P <= 1024 -> the 1024-thread form, footprint + 9 > 1024 -> k_fill_wide (two slots per thread).
SHAPES = {
    "base": (260, 4, 5150, 300),       # the base region: the band holds every level, footprint 249, P = 320
    "cmp": (400, 4, 345, 45),          # width 45 of test_every_strip_height: footprint 50, P = 64
    "w430": (520, 4, 730, 430),        # width 430 of test_every_strip_height: footprint ~450, P = 512 (too wide for the compact layout)
    "t1024": (640, 4, 730, 600),       # footprint ~600: P = 640
    "wide": (1090, 2, 83, 1000),       # the shortest of L = 1300, 1200, 1150, 1120, 1100, 1090 with P > 1024 (footprints 1025 and 1030; at 1080 they are 1017 and 1021, which round to 1024 slots)
    "sparse": (400, 4, 346, 300),      # ScoreMutations of ~20 edits keeps < 1/4 of the columns: the kept-column sweeps
}
FORM_OF = {"base": (257, 384), "cmp": (1, 256), "w430": (257, 512), "t1024": (513, 1024), "wide": (1025, 2048)}   # P in [lo, hi]


def shape(name):
    """(draft, events, params) of an ordinary region of SHAPES, made once"""
    if ("shape", name) not in _made:
        L, E, seed, width = SHAPES[name]
        par = dict(P0, realign_width=float(width))
        draft, events, _ = synth.make_region(L, E, seed, B.oracle_swalign, par)
        _made[("shape", name)] = (draft, events, par)
    draft, events, par = _made[("shape", name)]
    return draft, copy.deepcopy(events), dict(par)


def footprint(main):
    """rows between the first and the last in-band cell of the widest anti-diagonal i + j of a debug_fill matrix (NaN outside the band)"""
    i, j = np.nonzero(~np.isnan(main[1:, 1:]))
    s = i + j
    lo, hi = np.full(s.max() + 1, 1 << 30), np.full(s.max() + 1, -1)
    np.minimum.at(lo, s, i)
    np.maximum.at(hi, s, i)
    return int((hi - lo + 1).max())


def slots(width, realign_width):
    """P of a batch whose widest footprint is `width` (realign() and Batch::build / place, ps_host.cpp)"""
    w = max(width, 1)
    need = w + 9 if w + 9 <= 1024 else (w + 2 + 127) // 128 * 128
    pmax = max(64, min((2 * int(realign_width) + 10 + 63) // 64 * 64, 2048))
    return min(pmax, max(64, (need + 63) // 64 * 64))


def shape_edits(draft, n=20):
    """n random point edits and insertions of 2, 5, 20 and 40 bases: k_score's five size classes (7, 8, 16, 32 and 64 columns)"""
    muts = synth.random_point_mutations(np.random.default_rng(777), draft, n)
    q = len(draft) // 5
    return muts + [edit(q, "", "AC"), edit(2 * q, "", "ACGTA"), edit(3 * q, "", "ACGTA" * 4), edit(4 * q, draft[4 * q:4 * q + 1], "TGCA" * 10)]


def shape_tables(api, name, e, direction):
    draft, events, par = shape(name)
    h = api.align_create(draft, events, par)
    try:
        return api.debug_fill(h, e, direction, events[e].mean.size, len(draft) - 4)
    finally:
        api.align_destroy(h)


def live_forward_rows(fwd):
    """rows of a ViterbiMutate forward table before the first whose total is not a positive finite number (all of them: none is)"""
    tot = fwd.sum(axis=1)
    dead = np.flatnonzero(~(np.isfinite(tot) & (tot > 0)))
    return int(dead[0]) if dead.size else fwd.shape[0]
