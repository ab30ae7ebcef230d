"""Regions whose reads cover only part of them, shared by test_tiled.py (the oracle against the live reference, and the
preconditions that keep the crafted cases from going stale) and test_hip_tiled.py (the HIP path against the oracle).

`synth.make_region` walks every event over the whole truth sequence.  The reference's loader keeps every read that overlaps the
region by `min_overlap` bases, whole and overhanging (poreseq/LoadData.py:90-146, EventData.py:226-256), so at 10 kb regions most
reads start or stop inside the region.  `tiled_region` draws a genome with a margin on either side of the region and gives every
event its own span of it, in one of three representations of the part that lies outside:

  zeroed     whole level arrays, ref_align = 0 outside the region (what mapaligns' np.interp(..., 0, 0) leaves)
  truncated  level arrays cut to the aligned levels plus TRIM unaligned levels on either side
  loader     whole arrays, the overhang carried in region-relative coordinates: negative left of the region, greater than
             len(draft) right of it, continuing the end pairs linearly (what EventsFromBAM hands over after
             `aps[:,1] -= reginfo.start`; its pair list has no gap rows)

`synth.make_region`'s seeded streams are not touched: this module only calls synth's pieces.
"""
import copy

import numpy as np

import backends as B
from poreseq_amd import synth
from poreseq_amd.events import PSEvent
from poreseq_amd.util import DEFAULT_PARAMS, MutationInfo

P0 = dict(DEFAULT_PARAMS, verbose=0)
MODES = ("zeroed", "truncated", "loader")
TRIM = 7                       # unaligned levels kept on either side by "truncated"
VIT = (0.05, 0.01, 0.33, 0.75)   # Mutate's ViterbiMutate arguments (poreseq/Mutate.py)


def _extended(pairs, lo, hi):
    """gap-free (truth, draft) pairs continued linearly at both ends so that they cover truth indices lo .. hi"""
    pairs = pairs[(pairs[:, 0] > 0) & (pairs[:, 1] > 0)]
    (x0, y0), (x1, y1) = pairs[0], pairs[-1]
    head = [(x, y0 + (x - x0)) for x in range(min(lo, x0), x0)]
    tail = [(x, y1 + (x - x1)) for x in range(x1 + 1, max(hi, x1) + 1)]
    return np.array(head + [tuple(p) for p in pairs] + tail, dtype=np.int64).reshape(-1, 2)


def tiled_region(L, M, spans, seed, mode, params=None, swalign=None):
    """(draft, events, truth): a region of L bases inside a genome of L + 2 M, event k simulated over the genome bases of
    spans[k] = (s, t) in region coordinates (-M <= s < t <= L + M), its ref_align mapped onto the draft as `mode` says."""
    assert mode in MODES
    params = dict(P0 if params is None else params)
    swalign = B.oracle_swalign if swalign is None else swalign
    kids = np.random.SeedSequence(seed).spawn(len(spans) + 2)
    genome = synth.random_sequence(np.random.default_rng(kids[0]), L + 2 * M)
    truth = genome[M:M + L]
    draft = synth.corrupt(np.random.default_rng(kids[1]), truth, 0.04, 0.04, 0.04)
    pairs = np.array(swalign(truth, draft)[1], dtype=np.int64)
    events = []
    for e, (s, t) in enumerate(spans):
        assert -M <= s < t <= L + M, (s, t)
        rng = np.random.default_rng(kids[2 + e])
        piece = genome[s + M:t + M]
        model = synth.make_model(rng, complement=(e % 2 == 1))
        mean, stdv, ral = synth.simulate_event(rng, synth.states_of(piece), model)
        ev = PSEvent(mean, stdv, ral, np.zeros(mean.size), sequence=synth.corrupt(rng, piece, 0.05, 0.05, 0.05), model=model)
        ev.setparams(params)
        if mode == "loader":
            own = _extended(pairs, s + 1, t)
            own[:, 0] -= s                              # the read's own coordinates: all positive, as a BAM record's are
            ev.mapaligns(own)
        else:
            ev.ref_align = ev.ref_align + s             # region coordinates: <= 0 left of the region, > L right of it
            ev.mapaligns(pairs)
            if mode == "truncated":
                on = np.flatnonzero(ev.ref_align > 0)
                a, b = max(int(on[0]) - TRIM, 0), min(int(on[-1]) + TRIM + 1, ev.mean.size)
                for name in ("mean", "stdv", "ref_align", "ref_like"):
                    setattr(ev, name, getattr(ev, name)[a:b].copy())
                ev.makecontiguous()
        events.append(ev)
    return draft, events, truth


# name -> (L, M, params, spans, seed): the smallest shapes at which each mechanism can still fail (spans region-relative)
CRAFTED = {
    # Viterbi's stop branch in mid-region; two groups of refstart
    "gap": (400, 60, P0, ((-60, 170), (-20, 150), (10, 165), (250, 460), (240, 430), (260, 420)), 7101),
    # a stretch covered by one read: the skip branch on every skipped base
    "single": (400, 60, P0, ((-60, 460), (-30, 200), (20, 180), (150, 300), (0, 260)), 7102),
    # band pinned at rows 1.. and ..n0 for more than 1 024 columns (twice the four-wave model-row ring)
    "pinned": (1500, 100, dict(P0, realign_width=60.0), ((-100, 1600), (1100, 1600), (-100, 400), (600, 900), (1350, 1560)), 7103),
    # full-frame events (n0 < width) in the middle and at both ends
    "short": (1500, 100, P0, ((-100, 1600), (700, 860), (-50, 120), (1400, 1580)), 7104),
}
NAMES = tuple(CRAFTED)
PARTIAL = {"gap": 3, "single": 3, "pinned": 1, "short": 1}      # one partial event per case for the matrix comparisons

_made = {}


def _cached(key, make):
    if key not in _made:
        _made[key] = make()
    draft, events, params = _made[key]
    return draft, copy.deepcopy(events), dict(params)


def crafted(name, mode, swalign=None):
    """(draft, events, params) of a crafted case, made once per (name, mode, aligner)"""
    L, M, par, spans, seed = CRAFTED[name]
    return _cached((name, mode, swalign), lambda: tiled_region(L, M, spans, seed, mode, par, swalign)[:2] + (dict(par),))


def random_spans(seed):
    """(L, M, spans, params) of random_tiled(seed)"""
    rng = np.random.default_rng(88000 + seed)
    L, E, M = int(rng.integers(200, 421)), int(rng.integers(4, 9)), int(rng.integers(30, 151))
    spans = [(-M, L + M), (L // 3, L + M), (-M, 2 * L // 3)]
    while len(spans) < E:
        ln = int(rng.integers(L // 3, L + 1))
        s = int(rng.integers(max(-M, 40 - ln), min(L - 40, L + M - ln) + 1))      # at least 40 bases inside the region
        spans.append((s, s + ln))
    par = dict(P0, realign_width=40.0) if seed % 3 == 0 else dict(P0)
    return L, M, tuple(spans), par


def random_tiled(seed, mode, swalign=None):
    """(draft, events, params): L 200-420, E 4-8, M 30-150; one read over everything, one from L/3 overhanging the right end, one
    overhanging the left end up to 2L/3, the rest with random spans of L/3 .. L bases of which at least 40 lie inside the region;
    realign_width 40 on every third seed"""
    L, M, spans, par = random_spans(seed)
    return _cached(("random", seed, mode, swalign), lambda: tiled_region(L, M, spans, 88500 + seed, mode, par, swalign)[:2] + (par,))


def edit(start, orig, mut):
    mi = MutationInfo()
    mi.start, mi.orig, mi.mut = int(start), orig, mut
    return mi


def edits(draft, events, seed):
    """60 random point edits, then multi-base edits at the first and last covered base of every partial read, in the largest
    stretch that no read covers (if there is one) and at both ends of the region"""
    n = len(draft)
    muts = synth.random_point_mutations(np.random.default_rng(seed), draft, 60)
    cov = np.zeros(n + 2, dtype=np.int64)
    for ev in events:
        on = ev.ref_align[(ev.ref_align > 0) & (ev.ref_align <= n)]
        lo, hi = int(on[0]), int(on[-1])
        cov[lo:hi + 1] += 1
        if lo > 8 or hi < n - 8:
            for p in (lo - 1, hi - 1):
                p = min(max(p, 0), n - 6)
                muts += [edit(p, draft[p:p + 3], "AC"), edit(p, "", "GTTA"), edit(p, draft[p:p + 2], "")]
    bare = np.flatnonzero(cov[1:n + 1] == 0)
    if bare.size:
        runs = np.split(bare, np.flatnonzero(np.diff(bare) > 1) + 1)
        run = max(runs, key=len)
        p = min(int(run[len(run) // 2]), n - 8)
        muts += [edit(p, draft[p:p + 4], "T"), edit(p, "", "ACGTACG"), edit(p, draft[p:p + 1], "")]
    muts += [edit(0, "", "TT"), edit(0, draft[0:3], "G"), edit(1, draft[1:2], ""), edit(n - 5, draft[n - 5:n - 2], "CA"),
             edit(n - 1, draft[n - 1:], "A"), edit(n, "", "AC"), edit(n - 6, draft[n - 6:n - 2], "")]
    return muts


def band_rows(main):
    """(first row, last row) of the band in every column 1 .. C of a debug_fill matrix (rows = levels; NaN outside the band);
    columns without a band give (0, -1)"""
    inb = ~np.isnan(main[:, 1:])
    any_ = inb.any(axis=0)
    first = np.where(any_, inb.argmax(axis=0), 0)
    last = np.where(any_, main.shape[0] - 1 - inb[::-1].argmax(axis=0), -1)
    return first, last


def longest_run(mask):
    """length of the longest run of True"""
    best = cur = 0
    for m in mask:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return best


def fill_tables(api, draft, events, params, e, direction):
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        return api.debug_fill(h, e, direction, events[e].mean.size, len(draft) - 4)
    finally:
        api.align_destroy(h)


def viterbi_cap(draft, events):
    """rows enough for debug_viterbi.  ViterbiMutate walks from the smallest refstart to the largest refend, which the loader
    representation puts past the end of the draft, and then on for as long as a level of an unaligned tail sits on the position
    exactly: updaterefs continues the line through the first and last aligned level over the tail (cpp/EventData.h:146-153), so
    the walk can outrun the draft by the length of a zeroed overhang (random_tiled(5), zeroed, does).  No position lies past
    the end of that line."""
    top = float(len(draft))
    for ev in events:
        on = np.flatnonzero(ev.ref_align > 0)
        a0, a1 = int(on[0]), int(on[-1])
        slope = (ev.ref_align[a1] - ev.ref_align[a0]) / max(a1 - a0, 1)
        top = max(top, float(ev.ref_align.max()), float(ev.ref_align[a1] + abs(slope) * (ev.ref_align.size - 1 - a1)))
    return int(np.ceil(top)) + 64


def viterbi_tables(api, draft, events, params, nkeep, build=0):
    """debug_viterbi's tables of one region; the deviates come from the generator as B.reset_rand() leaves it"""
    B.reset_rand()
    h = api.align_create(draft, copy.deepcopy(events), params)
    try:
        return api.debug_viterbi([h], viterbi_cap(draft, events), nkeep, *VIT, obs_build=build)[0]
    finally:
        api.align_destroy(h)


def full_log(cls, draft, events, params):
    """every API result of one backend on a region: ScoreEvents, Coverage, ScorePoints, Mutate('viterbi', 2), Mutate('self', 2),
    Refine and the final ref_align / ref_like"""
    B.reset_rand()
    pa = B.make_pa(cls, draft, copy.deepcopy(events), params)
    log = [pa.ScoreEvents(), pa.Coverage().tolist(), [(s.start, s.orig, s.mut, s.score) for s in pa.ScorePoints()]]
    log += [pa.Mutate(seqs="viterbi", reps=2), pa.sequence]
    log += [pa.Mutate(reps=2), pa.sequence]
    log += [pa.Refine(), pa.sequence]
    log.append([e.ref_align.tolist() for e in pa.events])
    log.append([e.ref_like.tolist() for e in pa.events])
    return log


_oracle = {}


def oracle_once(key, make):
    """an oracle result computed once per session and handed out unchanged (callers must not write into it)"""
    if key not in _oracle:
        _oracle[key] = make()
    return _oracle[key]


# ---- tests/golden/tiled.npz: the reference's outputs on three cases (tests/golden/make_golden_tiled.py) -------------------------
GOLDEN_CASES = {"gap": "loader", "single": "truncated", "pinned": "truncated"}     # case -> representation recorded
GOLDEN_STORED = ("gap", "single")      # stored with their inputs; `pinned` is regenerated from its seed and checked by digest


def golden_inputs(name):
    """(draft, events, params) as recorded.  The stored cases keep their model tables as float16 (the file stays under the largest
    score fixture, 212 KB): the inputs are the crafted case with every model entry rounded to the nearest float16, which float64
    holds exactly."""
    draft, events, par = crafted(name, GOLDEN_CASES[name])
    if name in GOLDEN_STORED:
        for ev in events:
            for k in ("level_mean", "level_stdv", "sd_mean", "sd_stdv"):
                setattr(ev.model, k, np.asarray(getattr(ev.model, k), dtype=np.float16).astype(np.float64))
    return draft, events, par


def golden_outputs(cls, name, draft, events, par):
    """what the fixture records of one backend: ScoreEvents, ScoreMutations of `edits`, ScorePoints (stored cases), then
    Mutate('viterbi', 2), Mutate('self', 2), Refine with every count and sequence, and the SHA-256 of the final ref_align and ref_like"""
    import hashlib
    mk = lambda: B.make_pa(cls, draft, copy.deepcopy(events), par)
    out = {"ScoreEvents": np.array(mk().ScoreEvents()),
           "ScoreMutations": np.array([s.score for s in mk().ScoreMutations(edits(draft, events, 5))])}
    if name in GOLDEN_STORED:
        out["ScorePoints"] = np.array([s.score for s in mk().ScorePoints()])
    B.reset_rand()
    pa = mk()
    nb, seqs = [], []
    for call in (lambda: pa.Mutate(seqs="viterbi", reps=2), lambda: pa.Mutate(reps=2), pa.Refine):
        nb.append(call())
        seqs.append(pa.sequence)
    out["nbases"], out["sequences"] = np.array(nb), np.array(seqs)
    for e, ev in enumerate(pa.events):
        for k in ("ref_align", "ref_like"):
            out["final_ev%d_%s_sha256" % (e, k)] = np.array(hashlib.sha256(np.ascontiguousarray(getattr(ev, k), dtype=np.float64).tobytes()).hexdigest())
    return out


class _Sub:
    """the keys of one case of the fixture, without their prefix (what golden_util's loaders read)"""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix

    def __getitem__(self, k):
        return self.z[self.prefix + k]


def golden_load(name):
    """(draft, events, params, recorded outputs as a _Sub) of one case of tests/golden/tiled.npz"""
    import golden_util as G
    z = _Sub(G.load("tiled"), name + "/")
    if name in GOLDEN_STORED:
        draft, events, par = str(z["sequence"]), G.events_of(z), dict(G.params_of(z), verbose=0)
        for ev in events:
            ev.makecontiguous()
    else:
        draft, events, par = golden_inputs(name)
        if G.input_digest(draft, events, "") != str(z["input_sha256"]):
            raise AssertionError("generator drift: the regenerated inputs of %r do not match the fixture's checksum" % name)
    return draft, events, par, z


def check_golden(cls, name):
    draft, events, par, z = golden_load(name)
    got = golden_outputs(cls, name, draft, events, par)
    for k, v in got.items():
        want = z[k]
        if v.dtype.kind == "U":
            assert v.tolist() == [str(x) for x in want.tolist()] if want.ndim else str(v) == str(want), k
        else:
            assert np.array_equal(v, want), k
