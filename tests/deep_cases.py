"""Deep event stacks for the Viterbi emission kernels, and a plain restatement of the rule that combines the events of a position,
shared by test_deep_stacks.py (the oracle against the restatement, viterbi_ref and, when built, the live reference; the
preconditions that keep the stacks from going stale) and test_hip_deep_stacks.py (the three emission builds of ps_viterbi.hip
against all of them).

`trimmed_row` is cpp/Viterbi.cpp:327-349 in numpy and Python: ascending sort over the contributing events, the lowest quarter
dropped unless that leaves fewer than two, a serial sum from the lowest kept, the mean.  `restated_obs` puts it on the walk of
ref_cases.viterbi_positions and the rows of ref_cases.emission_row.

A stack of E events is made without a Smith-Waterman per read: the eight reads of one synthetic region copied round-robin, each
copy with its own perturbation of levels and stdvs (no two emissions equal), and its ref_align cut to zero behind its own position
as viterbi_cases.region does; the levels more than three behind the cut are dropped as well, because the reference finds a read
again on the extrapolated ref_index of such levels (`comes_back`).  The cuts lie on the positions that all eight reads have a level at, one copy per such position, so
that the number of contributing events falls from E to 1 one at a time: every count 1 .. E, and so every value of `drop`, occurs.
Copy 0 keeps everything.  `dup65` holds 32 pairs of exact copies (equal keys in the insertion sort), `flat73` is made of reads
without skips on the truth itself and is not cut: all of its positions have 73 contributors.

The builds' limits (ps_viterbi.hip): k_vit_obs_lds takes 72 events, k_vit_obs<64> 64, k_vit_obs<256> 256; E = 63 .. 65, 71 .. 73 and
255 .. 257 sit on either side of each."""
import copy
import math

import numpy as np

import backends as B
import ref_cases as RC
import viterbi_cases as K
from poreseq_amd import synth
from poreseq_amd.events import PSEvent

NS = 1024
BASE_E = 8
LEAD = 2                                 # positions with all eight reads before the first cut
SMALL = (260, 7301)                      # (L, seed) of the base region of the stacks up to 73 events
LARGE = (700, 7302)                      # ... of 255 and 256 events: long enough for 255 cuts (test_deep_stacks.py asserts it)
DEEP_E = (9, 30, 63, 64, 65, 71, 72, 73, 255, 256)
# name -> (events, base region, seed of the perturbations)
STACKS = {"E%d" % E: (E, SMALL if E <= 73 else LARGE, 7400 + E) for E in DEEP_E}
STACKS["dup65"] = (65, SMALL, 7501)
STACKS["flat73"] = (73, (120, 7303), 7502)
NAMES = tuple(STACKS)
REF_STACKS = ("E30", "E64", "E65", "E72", "E73", "dup65")          # the oracle against the live reference through Mutate
END_TO_END = ("E64", "E65", "E72", "E73", "dup65")                 # PSAlign against OraclePSAlign through Mutate
LDS_CAP = 72                             # events of the deepest region up to which a default call takes k_vit_obs_lds
COUNTERS = {1: "vit_obs_lds", 2: "vit_obs_64", 3: "vit_obs_256"}    # emission build -> launch counter (prof_get)
TOO_MANY = "more than 256 events"

_made = {}


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def drop_of(nl):
    """rows left out of the mean of nl: the lowest quarter, unless that leaves fewer than two"""
    drop = int(math.floor(nl * 0.25))
    return 0 if drop > nl - 2 else drop


def trimmed_row(rows):
    """[nl][1024] float64 -> [1024]: the trimmed mean over the events, in the reference's order of additions"""
    rows = np.asarray(rows, dtype=np.float64)
    nl = rows.shape[0]
    if nl == 1:
        return rows[0].copy()
    asc = np.sort(rows, axis=0)
    drop = drop_of(nl)
    acc = np.zeros(rows.shape[1])
    for k in range(drop, nl):                  # a serial sum from the lowest kept row (np.sum over a state's values adds pairwise)
        acc = acc + asc[k]
    return acc / float(nl - drop)


def restated_obs(events):
    """(walk of ref_cases.viterbi_positions, obs [T][1024]): for every kept position the trimmed_row of its contributors' rows"""
    walk = RC.viterbi_positions(events)
    obs = np.zeros((len(walk), NS))
    for t, (_, here) in enumerate(walk):
        obs[t] = trimmed_row(np.array([RC.emission_row(events[e].model, lvl, sd) for e, lvl, sd, _ in here]))
    return walk, obs


# ---- the stacks -------------------------------------------------------------------------------------------------------------------------
def base_region(L, seed):
    """(draft, eight events, positions that all eight have a level at, ascending)"""
    key = ("base", L, seed)
    if key not in _made:
        draft, events, _ = synth.make_region(L, BASE_E, seed, B.oracle_swalign, K.P0)
        # (an aligned level of its own: a hit on an interpolated level would go with the levels behind a cut)
        full = [refind for refind, here in RC.viterbi_positions(events)
                if len(here) == BASE_E and all(np.any(ev.ref_align == refind) for ev in events)]
        _made[key] = (draft, events, full)
    return _made[key]


def flat_region(L, seed):
    """(draft, eight events): reads that never skip, on the truth itself: every read has a level at every position"""
    key = ("flat", L, seed)
    if key not in _made:
        rng = np.random.default_rng(seed)
        truth = synth.random_sequence(rng, L)
        states = synth.states_of(truth)
        events = []
        for e in range(BASE_E):
            model = synth.make_model(rng, complement=(e % 2 == 1))
            mean, stdv, ral = synth.simulate_event(rng, states, model, p_skip=0.0)
            ev = PSEvent(mean, stdv, ral, np.zeros(mean.size), sequence=truth, model=model)
            ev.setparams(K.P0)
            events.append(ev)
        _made[key] = (truth, events)
    return _made[key]


def perturbed(ev, rng):
    """a copy of the event (the model shared) with its own levels and stdvs"""
    c = copy.copy(ev)
    n = ev.mean.size
    c.mean = ev.mean + rng.normal(0.0, 0.4, n)
    c.stdv = ev.stdv * np.exp(rng.normal(0.0, 0.08, n))
    c.ref_align, c.ref_like = ev.ref_align.copy(), ev.ref_like.copy()
    c.makecontiguous()
    return c


def twin(ev):
    """an exact copy (arrays of its own, the model shared)"""
    c = copy.copy(ev)
    for name in ("mean", "stdv", "ref_align", "ref_like"):
        setattr(c, name, getattr(ev, name).copy())
    return c


def comes_back(ra, position):
    """The reference extrapolates ref_index over the levels behind the last aligned one, along the line through the first and the
    last aligned level (cpp/EventData.h:131-141), and getrefstates takes a level whose extrapolated ref_index equals a position
    exactly.  The line's slope is a ratio of two small whole numbers, so a read whose ref_align was zeroed behind a position
    is found again further on, every (levels between its first and last aligned one) levels.  True where an extrapolated value
    behind the last aligned level of `ra` is a whole number above `position`."""
    on = np.flatnonzero(ra > 0)
    if on.size < 2:
        return False                 # one aligned level: slope 0 / 0, every extrapolated value NaN
    a, b = int(on[0]), int(on[-1])
    m = (ra[b] - ra[a]) / np.float64(b - a)
    tail = m * np.arange(b + 1, ra.size, dtype=np.float64) + (ra[a] - m * a)
    return bool(np.any((tail == np.floor(tail)) & (tail > position)))


TAIL = 3                                 # unaligned levels a cut read keeps behind its last aligned one


def cut_behind(ev, position):
    """ref_align to zero behind the position, as viterbi_cases.region does, and the levels more than TAIL behind the last aligned
    one dropped (fewer where even those would come back): the read contributes nowhere behind its cut"""
    ra = np.where(ev.ref_align > position, 0.0, ev.ref_align)
    on = np.flatnonzero(ra > 0)
    assert on.size, "no aligned level up to position %d" % position
    for tail in range(TAIL, -1, -1):
        n = min(ra.size, int(on[-1]) + 1 + tail)
        if not comes_back(ra[:n], position):
            break
    ev.ref_align = ra
    RC.levels_cut([ev], n)
    return ev


def _build(name):
    E, (L, seed), pseed = STACKS[name]
    rng = np.random.default_rng(pseed)
    if name == "flat73":
        draft, base = flat_region(L, seed)
        return draft, [perturbed(base[k % BASE_E], rng) for k in range(E)]
    draft, base, full = base_region(L, seed)
    assert len(full) >= LEAD + E - 1, "%s: %d positions with all reads, %d needed: lengthen the region" % (name, len(full), LEAD + E - 1)
    if name == "dup65":
        events = []
        for i in range(32):
            one = perturbed(base[i % BASE_E], rng)
            events += [one, twin(one)]
        events.append(perturbed(base[0], rng))
    else:
        events = [perturbed(base[k % BASE_E], rng) for k in range(E)]
    for k in range(1, E):          # copy k contributes up to the (E - 1 - k)-th cut position: E - j contributors at cut position j
        cut_behind(events[k], full[LEAD + E - 1 - k])
    return draft, events


def stack(name):
    """(draft, events) of a stack; made once, handed out as a copy"""
    if name not in _made:
        _made[name] = _build(name)
    draft, events = _made[name]
    return draft, copy.deepcopy(events)


def stack257():
    """the 256-event stack with one more perturbed copy: more than any build takes"""
    draft, events = stack("E256")
    base = base_region(*LARGE)[1]
    return draft, events + [perturbed(base[0], np.random.default_rng(7600))]


EMPTY_DRAFT_SEED = 7700


def empty_region():
    """a region without events"""
    return synth.random_sequence(np.random.default_rng(EMPTY_DRAFT_SEED), 80), []


def no_positions_region():
    """three reads whose walk keeps no position (ref_cases' all_unaligned): T = 0.  The Viterbi entry points refuse an AlignData
    without events, alone or in a batch, so this region stands in the middle of the batches of handles."""
    draft, events, _ = RC.case("all_unaligned")
    return draft, events


MIXED_E = (1, 73, 0, 9, 72)


def mixed_batch(with73=True, middle="empty"):
    """[(draft, events)] with E = (1, 73, 0, 9, 72), or with the region without positions in the middle (E = 3, T = 0); without
    the 73-event member the deepest region has 72 events: the LDS build"""
    one = K.region(*K.REGIONS[0])
    regs = [one, stack("E73"), empty_region() if middle == "empty" else no_positions_region(), stack("E9"), stack("E72")]
    return regs if with73 else regs[:1] + regs[2:]


def batch_cap(regs):
    return max(len(d) for d, _ in regs) + 64


def short_edits(draft, seed):
    """a short seeded list of point edits"""
    return synth.random_point_mutations(np.random.default_rng(seed), draft, 6)


def duplicate_pairs():
    return [(2 * i, 2 * i + 1) for i in range(32)]


# ---- computed once per session --------------------------------------------------------------------------------------------------------------
def restated(name):
    return RC.once(("deep restated", name), lambda: restated_obs(stack(name)[1]))


def oracle_tables(name, nkeep):
    def make():
        draft, events = stack(name)
        return RC.viterbi_tables(B.oracle_api(), draft, events, K.P0, nkeep, len(draft) + 64)
    return RC.once(("deep oracle", name, nkeep), make)


def steps_ref(name):
    """viterbi_ref.run64 on the restated rows"""
    import viterbi_ref as V
    return RC.once(("deep run64", name), lambda: V.run64(restated(name)[1], K.SKIP, K.STAY))


def expected_build(E):
    """the build a default call takes for a deepest region of E events"""
    return 1 if E <= LDS_CAP else 3
