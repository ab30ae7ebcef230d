"""Caller-written ref_align arrays and a plain restatement of what the reference makes of them, shared by test_ref_tables.py (the
oracle against the restatement and, when built, the live reference; the preconditions that keep the crafted arrays from going
stale) and test_hip_ref_tables.py (the HIP path against the oracle and the restatement).

`ref_tables` is cpp/EventData.h:110-204 as plain loops over float64 (updaterefs, getrefstate, getrefstates), written from the
reference and not from the oracle.  `band_mask` puts the bands of a fill on it (cpp/Alignment.cpp:127-148 / :299-323, the rule
ps_debug.cpp states for its un-skewing), `viterbi_positions` the walk of ViterbiMutate over the reference positions
(cpp/Viterbi.cpp:261-325) and `emission_row` the emission of a position that one event alone contributes to.

The crafted families write arrays that synth's alignments never hold: an un-interpolated hole behind an aligned level 0 (the
reference's `lastal > 0`), holes laid on the thread chunks of k_updaterefs (ceil(n / 256) levels per thread), one aligned level
(slope 0 / 0: ref_index is NaN), two aligned levels on one column (slope 0), back steps (ref_index unsorted: the bisection path
decides the band), -1 / 0 / NaN markers, fractional values, values in (0, 1), values past the end of the sequence, long runs on
one column, reads without an aligned level, a read of 0 levels, a region of one read.  Level counts are N in {0, 1, 2, 255, 256,
257, 513, 1025}: chunk 0, 1, 1, 1, 1, 2, 3, 5.

Domain: an aligned entry is below 2^31 (include/poreseq_hip.h); the largest entry here is 20000, because ViterbiMutate's position
loop is linear in it."""
import copy
import math

import numpy as np

import backends as B
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS, MutationInfo

P0 = dict(DEFAULT_PARAMS, verbose=0)
WIDTHS = (3, 20, 300)           # narrower than most distortions; ordinary; the default (n0 < W on the short reads)
VIT = (0.05, 0.01, 0.33, 0.75)  # Mutate's ViterbiMutate arguments (poreseq/Mutate.py)
THREADS = 256                   # of k_updaterefs
NS = 1024
LOG2PI = math.log(2 * math.pi)  # cpp/AlignUtil.h:24


def chunk_of(n):
    """levels per thread of k_updaterefs"""
    return (n + THREADS - 1) // THREADS


# ---- cpp/EventData.h:110-204 ----------------------------------------------------------------------------------------------------------
class RefTables:
    """updaterefs of one ref_align array, and the two look-ups.  ref_index is None when no level is aligned (the reference's empty
    vector).  Beside the tables, what the loop went through: `sic` (an aligned level met with lastal == 0 behind a hole: the hole
    stays as it is), `interpolated` (the levels a hole interpolation wrote), `holes` ((first, last + 1) of every run of unaligned
    levels between the first and the last aligned one)."""

    def __init__(self, ra):
        ra = [float(x) for x in ra]
        n = len(ra)
        self.ra, self.n = ra, n
        self.refstart = self.refend = -1
        self.ref_index = None
        self.sic, self.interpolated, self.holes = False, set(), []
        ra0 = 0
        while ra0 < n and not ra[ra0] > 0:
            ra0 += 1
        ra1 = n - 1
        while ra1 >= 0 and not ra[ra1] > 0:
            ra1 -= 1
        if ra0 == n or ra1 < 0:
            return
        self.first, self.last = ra0, ra1
        self.refstart, self.refend = int(ra[ra0]), int(ra[ra1])       # (int): towards zero; the domain keeps it defined
        ri = list(ra)
        with np.errstate(all="ignore"):
            al_m = float(np.float64(ra[ra1] - ra[ra0]) / np.float64(ra1 - ra0))      # 0 / 0 = NaN when one level is aligned
        al_b = ra[ra0] - al_m * ra0
        lastal = -1
        for i in range(n):
            if i < ra0 or i > ra1:
                ri[i] = al_m * i + al_b
            elif ra[i] > 0:
                if lastal >= 0 and i - lastal > 1:
                    self.holes.append((lastal + 1, i))
                if lastal > 0:
                    m = (ra[i] - ra[lastal]) / (i - lastal)
                    for j in range(lastal + 1, i):
                        ri[j] = m * (j - lastal) + ra[lastal]
                        self.interpolated.add(j)
                elif lastal == 0 and i > 1:
                    self.sic = True
                lastal = i
        self.ref_index = ri
        self._first = None

    def getrefstate(self, j):
        """std::lower_bound as libstdc++ walks it (bits/stl_algobase.h, __lower_bound): on an unsorted array or one with NaN the
        answer is whatever this walk arrives at"""
        if self.ref_index is None:
            return 0
        a, first, length = self.ref_index, 0, self.n
        while length > 0:
            half = length >> 1
            mid = first + half
            if a[mid] < j:
                first = mid + 1
                length = length - half - 1
            else:
                length = half
        return first

    def find(self, r):
        """std::find(ref_index, r): the first level whose ref_index == r, or None.  (A dictionary of first occurrences: == on
        doubles is dictionary equality for every value but NaN, which equals nothing and is left out.)"""
        if self.ref_index is None:
            return None
        if self._first is None:
            self._first = {}
            for i, v in enumerate(self.ref_index):
                if v == v and v not in self._first:
                    self._first[v] = i
        return self._first.get(r)

    def getrefstates(self, r):
        i = self.find(r)
        if i is None:
            return []
        inds = [i]
        i += 1
        while i < self.n and self.ra[i] <= r:
            if self.ra[i] > 0:
                inds.append(i)
            i += 1
        return inds

    # what the generators claim, read off the tables
    def unsorted(self):
        v = [x for x in (self.ref_index or []) if x == x]
        return any(a > b for a, b in zip(v, v[1:]))

    def has_nan(self):
        return any(x != x for x in (self.ref_index or []))

    def whole_chunk_hole(self):
        """a hole holds at least one whole thread chunk of k_updaterefs"""
        c = chunk_of(self.n)
        return any((-(-a // c) + 1) * c <= b for a, b in self.holes)


def ref_tables(ra):
    return RefTables(ra)


def band_mask(ra, n0, C, W, direction):
    """bool [n0 + 1][C + 1]: the cells a fill holds.  Column 0 is the blank column, all rows; a read without an aligned level has
    no other column.  Column c = 1 .. C is centred on getrefstate(c) forward, on n0 - getrefstate(C - c + 1) + 1 backward, the
    centre clamped to 1 .. n0, W rows on either side."""
    t = ra if isinstance(ra, RefTables) else ref_tables(ra)
    mask = np.zeros((n0 + 1, C + 1), dtype=bool)
    mask[:, 0] = True
    if t.ref_index is None or W == 0:
        return mask
    for c in range(1, C + 1):
        ce = t.getrefstate(c) if direction == 0 else n0 - t.getrefstate(C - c + 1) + 1
        ce = min(max(ce, 1), n0)
        mask[max(1, ce - W):min(n0, ce + W) + 1, c] = True
    return mask


def viterbi_positions(events, limit=200000):
    """The positions ViterbiMutate keeps (cpp/Viterbi.cpp:261-325): [(refind, [(event, mean level, mean stdv, first level of the
    hit), ...])].  A position is kept unless nl <= 0.2 * nal; the walk stops when it is not kept and nal == 0."""
    tabs = [ref_tables(ev.ref_align) for ev in events]
    refind = tabs[0].refstart
    for t in tabs:
        refind = min(refind, t.refstart)
    kept = []
    for _ in range(limit):
        here = []
        for e, (t, ev) in enumerate(zip(tabs, events)):
            inds = t.getrefstates(refind)
            if not inds:
                continue
            lvl = sd = 0.0
            for i in inds:
                lvl += float(ev.mean[i])
                sd += float(ev.stdv[i])
            here.append((e, lvl / len(inds), sd / len(inds), inds[0]))
        nal = sum(1 for t in tabs if t.refstart <= refind <= t.refend)
        if len(here) <= nal * 0.2:
            if nal == 0:
                return kept
            refind += 1
            continue
        kept.append((refind, here))
        refind += 1
    raise AssertionError("the walk did not stop within %d positions" % limit)


def emission_row(model, lvl, sd):
    """the 1024 emissions of one event's (mean level, mean stdv) at a position (cpp/Viterbi.cpp:300-306, cpp/AlignUtil.h:34-53);
    logarithms and powers through libm (math), everything else elementwise IEEE"""
    key = id(model)
    if key not in _model_logs:
        lm, ls = np.asarray(model.level_mean, dtype=np.float64), np.asarray(model.level_stdv, dtype=np.float64)
        sm, ss = np.asarray(model.sd_mean, dtype=np.float64), np.asarray(model.sd_stdv, dtype=np.float64)
        # pow(sd_mean, 3) / pow(sd_stdv, 2), cpp/EventData.h:61: the compilers in use expand pow(x, 2) to x * x (not always libm's bits)
        lam = np.array([math.pow(a, 3) / (b * b) for a, b in zip(sm.tolist(), ss.tolist())])
        _model_logs[key] = (model, lm, ls, np.array([math.log(x) for x in ls.tolist()]), sm, lam, np.array([math.log(x) for x in lam.tolist()]))
    _, lm, ls, log_lev, sm, lam, log_lam = _model_logs[key]
    d = (lvl - lm) / ls
    out = -0.5 * (d * d + LOG2PI) - log_lev
    d = (sd - sm) / sm
    out = out + 0.5 * (log_lam - 3 * math.log(sd) - LOG2PI - d * d * lam / sd)
    return out


_model_logs = {}


# ---- events -----------------------------------------------------------------------------------------------------------------------
PER_LEVEL = ("mean", "stdv", "length", "start", "ref_align", "ref_like")


def levels_cut(events, n):
    """every per-level array of every event cut to exactly n levels (n: one count, or one per event), in place"""
    ns = [n] * len(events) if isinstance(n, int) else list(n)
    for ev, k in zip(events, ns):
        assert ev.mean.size >= k, (ev.mean.size, k)
        for name in PER_LEVEL:
            if hasattr(ev, name):
                setattr(ev, name, np.array(getattr(ev, name)[:k], dtype=np.float64))
        ev.makecontiguous()
    return events


def _near(orig, i):
    """the value of the aligned level of `orig` nearest to i, looking back first (column i + 1 when a short cut holds none)"""
    for j in list(range(i, -1, -1)) + list(range(i + 1, len(orig))):
        if orig[j] > 0:
            return float(orig[j])
    return float(i + 1)


def _pin(ra, orig, i):
    """level i aligned (with its own value, or its neighbour's)"""
    if not ra[i] > 0:
        ra[i] = _near(orig, i)


# Every family: f(ra, orig, k) writes into ra (float64 [N], a copy of orig = synth's array cut to N levels); k = index of the read
def sic_hole(ra, orig, k):
    """level 0 aligned, levels 1 .. h unaligned (h = 1 on read 0, 3 chunks + 1 on the others): not interpolated.  A second hole
    later on is interpolated, laid between two anchors as many columns apart as levels, so that its interpolated ref_index are
    integers no aligned level holds: getrefstates' hits fall on interpolated levels"""
    n, c = ra.size, chunk_of(ra.size)
    h = 1 if k == 0 else 3 * c + 1
    _pin(ra, orig, 0)
    ra[1:h + 1] = 0.0
    _pin(ra, orig, h + 1)
    for a in range(max(n // 2, h + 3), n - 4):
        if not orig[a - 1] > 0:
            continue
        for b in range(a + 2, min(a + 12, n)):
            if orig[b] > 0 and orig[b] - orig[a - 1] == b - (a - 1):
                ra[a:b] = 0.0
                return
    raise AssertionError("no place for a hole with integer interpolation")


def chunk_holes(ra, orig, k):
    """four holes on the thread chunks: one whole chunk; four whole chunks plus a level on either side; one that ends on the last
    level of a chunk (and starts inside it when the chunk has room); one that starts on the first level of a chunk"""
    c = chunk_of(ra.size)
    holes = [(10 * c, 11 * c), (20 * c - 1, 24 * c + 1), (30 * c + c // 2 if c > 1 else 29, 31 * c), (40 * c, 40 * c + max(1, c // 2))]
    for a, b in holes:
        ra[a:b] = 0.0
        _pin(ra, orig, a - 1)
        _pin(ra, orig, b)


def late_first(ra, orig, k):
    """the first aligned level lies in the chunk of the last thread that has levels"""
    c = chunk_of(ra.size)
    t0 = ((ra.size - 1) // c) * c
    ra[:t0] = 0.0
    for i in range(t0, ra.size):
        _pin(ra, orig, i)


def early_last(ra, orig, k):
    """the last aligned level lies in thread 0's chunk"""
    c = chunk_of(ra.size)
    ra[c:] = 0.0
    for i in range(c):
        ra[i] = _near(orig[::-1], ra.size - 1 - i) if not orig[i] > 0 else orig[i]


def _single(at):
    def f(ra, orig, k):
        i = {"0": 0, "mid": ra.size // 2, "last": ra.size - 1}[at]
        v = _near(orig, i)
        ra[:] = 0.0
        ra[i] = v
    f.__doc__ = "exactly one aligned level (%s): slope 0 / 0" % at
    return f


def two_equal(ra, orig, k):
    """two aligned levels on one column, far apart: slope 0"""
    n = ra.size
    v = _near(orig, n // 2)
    ra[:] = 0.0
    ra[n // 8], ra[n - 1 - n // 8] = v, v


def back_steps(ra, orig, k):
    """a stretch of 25 levels moved 40 columns back"""
    s = slice(ra.size // 2, ra.size // 2 + 25)
    ra[s] = np.where(ra[s] > 40, ra[s] - 40, ra[s])


def reversed_array(ra, orig, k):
    """read 0 and 1: the whole array reversed (levels stay as they are)"""
    if k < 2:
        ra[:] = orig[::-1]


def markers(ra, orig, k):
    """-1, 0 and NaN in the un-interpolated head behind an aligned level 0, inside an interpolated hole and in the tail"""
    n, nan = ra.size, float("nan")
    _pin(ra, orig, 0)
    ra[1:9] = [-1, -1, 0, nan, nan, -1, 0, -1]
    _pin(ra, orig, 9)
    a = n // 3
    _pin(ra, orig, a - 1)
    ra[a:a + 6] = [-1, 0, nan, -1, -1, 0]
    _pin(ra, orig, a + 6)
    _pin(ra, orig, n - 13)
    ra[n - 12:] = [-1, nan, 0, -1] * 3


def fractional(ra, orig, k):
    """+0.5 on 40 aligned levels; further on an x.0 between (x - 1).999 and x.999"""
    n = ra.size
    s = slice(n // 4, n // 4 + 40)
    ra[s] = np.where(ra[s] > 0, ra[s] + 0.5, ra[s])
    i = (3 * n) // 4
    x = math.floor(_near(orig, i))
    ra[i - 1], ra[i], ra[i + 1] = x - 1 + 0.999, float(x), x + 0.999


def column0(ra, orig, k):
    """values in (0, 1) on the first levels: aligned, column 0 (refstart = 0)"""
    m = min(3, ra.size)
    ra[:m] = [0.25, 0.5, 0.999][:m]


def past_end(ra, orig, k):
    """the last 30 aligned levels + 500 (reads 0 and 2); one entry of 20000 (reads 1 and 2)"""
    on = np.flatnonzero(ra > 0)
    if k != 1:
        ra[on[-30:]] += 500.0
    if k != 0:
        ra[on[-1]] = 20000.0


def long_run(ra, orig, k):
    """80 levels on one column"""
    a = ra.size // 3
    ra[a:a + 80] = _near(orig, a)


def unaligned_middle(ra, orig, k):
    """read 1 without an aligned level, next to live reads"""
    if k == 1:
        ra[:] = 0.0


def unaligned_first_markers(ra, orig, k):
    """read 0 without an aligned level (ViterbiMutate starts from events[0].refstart = -1) next to a read whose ref_index holds
    -1: the un-interpolated markers behind its aligned level 0, which std::find(ref_index, -1) meets at position -1"""
    if k == 0:
        ra[:] = 0.0
    elif k == 1:
        _pin(ra, orig, 0)
        ra[1:4] = [-1, 0, -1]
        _pin(ra, orig, 4)


def empty_read(ra, orig, k):
    """read 0 has no levels at all (refstart = -1: the walk starts at -1); the live reads begin on column 0, so that a read is
    aligned at position 0 and the walk goes on from there (where it ends at once the reference is not defined: all_unaligned)"""
    if ra.size:
        column0(ra, orig, k)


def untouched(ra, orig, k):
    """synth's own arrays cut to N levels"""


# name -> (family, level counts of the reads, seed)
FAMILIES = {
    "sic_hole": (sic_hole, (257, 513, 1025), 9101),
    "chunk_holes": (chunk_holes, (257, 513, 1025), 9102),
    "late_first": (late_first, (256, 257, 513), 9103),
    "early_last": (early_last, (256, 257, 513), 9104),
    "single_at_0": (_single("0"), (1, 257, 513), 9105),
    "single_mid": (_single("mid"), (2, 256, 257), 9106),
    "single_last": (_single("last"), (2, 257, 513), 9107),
    "two_equal": (two_equal, (2, 256, 513), 9108),
    "back_steps": (back_steps, (255, 257, 513), 9109),
    "reversed": (reversed_array, (256, 257, 255), 9110),
    "markers": (markers, (256, 257, 513), 9111),
    "fractional": (fractional, (255, 256, 257), 9112),
    "column0": (column0, (2, 255, 257), 9113),
    "past_end": (past_end, (255, 256, 257), 9114),
    "long_run": (long_run, (255, 257, 513), 9115),
    "all_unaligned": (unaligned_middle, (1, 256, 257), 9116),
    "unaligned_markers": (unaligned_first_markers, (2, 255, 257), 9117),
    "untouched": (untouched, (1, 256, 513), 9118),
    "empty_read": (empty_read, (0, 255, 257), 9119),
    "one_read": (markers, (257,), 9120),        # every kept position has one contributor: every emission row is restated
}
ONE_READ = ("one_read",)
NAMES = tuple(FAMILIES)
# what each family is asserted to reach (test_ref_tables.py): attribute of RefTables -> families
REACH = {
    "sic": ("sic_hole", "markers", "unaligned_markers"),
    "whole_chunk_hole": ("chunk_holes", "sic_hole"),
    "unsorted": ("back_steps", "reversed"),
    "has_nan": ("single_at_0", "single_mid", "single_last", "late_first"),
}
INTERP_HIT = ("sic_hole",)      # a getrefstates hit of the Viterbi walk falls on an interpolated level

_made = {}


def base_region(counts, seed):
    """(draft, events): a synth region long enough for the largest count, read k cut to counts[k] levels"""
    L = int(max(counts) * 1.12) + 30
    draft, events, _ = synth.make_region(L, len(counts), seed, B.oracle_swalign, P0)
    return draft, levels_cut(copy.deepcopy(events), counts)


def apply_family(events, family):
    for k, ev in enumerate(events):
        orig = ev.ref_align.copy()
        ra = orig.copy()
        family(ra, orig, k)
        ev.ref_align = ra
        ev.makecontiguous()


def crafted():
    """name -> (draft, events, params); made once, handed out as copies"""
    if "crafted" not in _made:
        out = {}
        for name, (family, counts, seed) in FAMILIES.items():
            draft, events = base_region(counts, seed)
            apply_family(events, family)
            out[name] = (draft, events, dict(P0))
        _made["crafted"] = out
    return {k: (d, copy.deepcopy(e), dict(p)) for k, (d, e, p) in _made["crafted"].items()}


def case(name):
    """(draft, events, params) of a crafted family or of ("random", seed)"""
    if isinstance(name, tuple):
        return random_case(name[1])
    crafted()
    d, e, p = _made["crafted"][name]
    return d, copy.deepcopy(e), dict(p)


# ---- random cases -----------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = tuple(range(12))
RANDOM_GPU = RANDOM_SEEDS[:6]


def _rand_hole(rng, ra, orig, k):
    n = ra.size
    a = int(rng.integers(0, n))
    ra[a:a + int(rng.integers(1, 4 * chunk_of(n) + 3))] = rng.choice([0.0, -1.0, float("nan")])


def _rand_back(rng, ra, orig, k):
    a = int(rng.integers(0, ra.size))
    s = slice(a, a + int(rng.integers(1, 30)))
    d = float(rng.integers(1, 60))
    ra[s] = np.where(ra[s] > d, ra[s] - d, ra[s])


def _rand_frac(rng, ra, orig, k):
    a = int(rng.integers(0, ra.size))
    s = slice(a, a + int(rng.integers(1, 40)))
    ra[s] = np.where(ra[s] > 0, ra[s] + rng.choice([0.5, 0.999, 0.25]), ra[s])


def _rand_run(rng, ra, orig, k):
    a = int(rng.integers(0, ra.size))
    ra[a:a + int(rng.integers(2, 90))] = _near(orig, a)


def _rand_past(rng, ra, orig, k):
    on = np.flatnonzero(ra > 0)
    if on.size:
        ra[on[-int(rng.integers(1, 31)):]] += float(rng.integers(1, 600))


def _rand_col0(rng, ra, orig, k):
    m = min(int(rng.integers(1, 4)), ra.size)
    ra[:m] = rng.uniform(0.01, 0.99, m)


def _rand_head(rng, ra, orig, k):
    """an aligned level 0 and markers behind it"""
    h = min(int(rng.integers(1, 3 * chunk_of(ra.size) + 3)), ra.size - 1)
    _pin(ra, orig, 0)
    ra[1:1 + h] = rng.choice([0.0, -1.0, float("nan")], h)


def _rand_few(rng, ra, orig, k):
    """zero to three aligned levels"""
    keep = rng.integers(0, ra.size, int(rng.integers(0, 4)))
    vals = [_near(orig, int(i)) for i in keep]
    ra[:] = 0.0
    for i, v in zip(keep, vals):
        ra[int(i)] = v


def _rand_reverse(rng, ra, orig, k):
    ra[:] = ra[::-1].copy()


RANDOM_OPS = (_rand_hole, _rand_hole, _rand_back, _rand_frac, _rand_run, _rand_past, _rand_col0, _rand_head, _rand_few, _rand_reverse)


def random_case(seed):
    """(draft, events, params): 2 or 3 reads of 1 .. 600 levels, each with one to four of the operations above in a row"""
    key = ("random", seed)
    if key not in _made:
        rng = np.random.default_rng(97000 + seed)
        counts = [int(rng.choice([int(rng.integers(1, 5)), int(rng.integers(250, 262)), int(rng.integers(5, 601))])) for _ in range(int(rng.integers(2, 4)))]
        counts[0] = max(counts[0], 40)          # one read that a region can be built around
        draft, events = base_region(counts, 97500 + seed)
        for k, ev in enumerate(events):
            orig = ev.ref_align.copy()
            ra = orig.copy()
            for _ in range(int(rng.integers(1, 5))):
                RANDOM_OPS[int(rng.integers(0, len(RANDOM_OPS)))](rng, ra, orig, k)
            ev.ref_align = ra
            ev.makecontiguous()
        _made[key] = (draft, events, dict(P0))
    d, e, p = _made[key]
    return d, copy.deepcopy(e), dict(p)


ALL_CASES = NAMES + tuple(("random", s) for s in RANDOM_SEEDS)
GPU_CASES = NAMES + tuple(("random", s) for s in RANDOM_GPU)


def case_id(c):
    return c if isinstance(c, str) else "random%d" % c[1]


# ---- what the tests run --------------------------------------------------------------------------------------------------------------
def edit(start, orig, mut):
    mi = MutationInfo()
    mi.start, mi.orig, mi.mut = int(start), orig, mut
    return mi


def edits(draft, seed=5):
    """20 edits: 12 random point edits and multi-base edits at both ends of the region"""
    n = len(draft)
    muts = synth.random_point_mutations(np.random.default_rng(seed), draft, 12)
    muts += [edit(0, "", "TT"), edit(0, draft[0:3], "G"), edit(1, draft[1:2], ""), edit(n - 5, draft[n - 5:n - 2], "CA"),
             edit(n - 1, draft[n - 1:], "A"), edit(n, "", "AC"), edit(n - 6, draft[n - 6:n - 2], ""), edit(2, draft[2:4], "ACG")]
    return muts


def with_width(params, W):
    return dict(params, realign_width=float(W))


def fill_tables(api, draft, events, params, e, direction):
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        return api.debug_fill(h, e, direction, events[e].mean.size, len(draft) - 4)
    finally:
        api.align_destroy(h)


def viterbi_tables(api, draft, events, params, nkeep, cap, build=0):
    """debug_viterbi's tables of one region, room for `cap` positions; the deviates come from the generator as B.reset_rand() leaves it"""
    B.reset_rand()
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        return api.debug_viterbi([h], cap, nkeep, *VIT, obs_build=build)[0]
    finally:
        api.align_destroy(h)


def refs(pa):
    return [ev.ref_align.copy() for ev in pa.events] + [ev.ref_like.copy() for ev in pa.events]


def same_arrays(a, b):
    """equal arrays, NaN equal to NaN (a ref_align that no call rewrote keeps the caller's NaN markers)"""
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


_once = {}


def once(key, make):
    """a result computed once per session and handed out unchanged (callers must not write into it)"""
    if key not in _once:
        _once[key] = make()
    return _once[key]
