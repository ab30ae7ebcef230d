"""Inputs of the Viterbi table tests, shared by the CPU module (oracle hooks against viterbi_ref, and the preconditions that keep
the crafted inputs from going stale) and the GPU module (the HIP kernels against both)."""
import copy

import numpy as np

import backends as B
import viterbi_ref as V
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS

SKIP, STAY, MMIN, MMAX = 0.05, 0.01, 0.33, 0.75      # Mutate's ViterbiMutate arguments (poreseq/Mutate.py)
P0 = dict(DEFAULT_PARAMS, verbose=0)
NS = V.NS

# every phase of the 4 + 4 unrolled loop of k_vit_steps and of its prefetch clamp, one and several loop trips
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)
# (first row, last row, shift in nats): a stretch of rows whose emissions all drop; the reference's exp(obs) and fs * exp(obs)
# stay normal in all of them (obs > -400 everywhere, float64 underflows at -708)
TROUGHS = ((9, 29, -20.0), (9, 29, -60.0), (9, 29, -150.0), (9, 29, -300.0), (0, 6, -100.0))
TROUGH_T = 40


def random_rows(T, seed):
    """obs = -2.5 - Gamma(2, 3) per state: the magnitudes of real trimmed-mean emissions"""
    return -2.5 - np.random.default_rng(seed).gamma(2.0, 3.0, (T, NS))


def trough_rows(case):
    lo, hi, shift = case
    rows = random_rows(TROUGH_T, 500 + int(-shift))
    rows[lo:hi + 1] += shift
    return rows


def tie_rows():
    """Rounding ties: after row 0 every 1-base family {g, g + 256, g + 512, g + 768} holds its maximum at g + 256, one ulp above
    member g, the other two 1 and 2 nats lower.  Row 1 has ordinary magnitudes, so about half of its sums a + lik[g] and
    a + lik[g + 256] round to the same double and the reference's ordered scan keeps g, the first it met."""
    rng = np.random.default_rng(77)
    rows = random_rows(3, 78)
    b = rng.uniform(-6.4, -4.2, 256)      # b + log .25 stays inside [-8, -4): one ulp apart before the step is one ulp apart after
    rows[0, 0:256] = b
    rows[0, 256:512] = np.nextafter(b, np.inf)
    rows[0, 512:768] = b - 1.0
    rows[0, 768:1024] = b - 2.0
    return rows


def equal_rows():
    """Exact ties: all 1024 emissions equal for nine rows, so every family ties fully on every step"""
    return np.full((9, NS), -3.25)


# ---- rows that kill the max-plus vector, wholly or partly.  k_vit_steps starts every maximum at -1e300 with back-pointer -1 (as the
# reference): a state none of whose candidates is above -1e300 keeps both, and once a whole row has, every later sum rounds back to
# -1e300 and every later row is dead too.  name -> (T, [(rows, states, value)], back-pointers of -1 per row)
DEAD_BASE = (9, 7)                     # random_rows(T, seed)
_ALL, _EVEN, _ODD = slice(None), slice(0, None, 2), slice(1, None, 2)
_MID = (0, 0, 0, 0, 1024, 1024, 1024, 1024, 1024)
DEAD_CASES = {
    "neginf_mid": (9, [(4, _ALL, -np.inf)], _MID),
    "neginf_first": (9, [(0, _ALL, -np.inf)], (1024,) * 9),
    "neginf_last": (9, [(8, _ALL, -np.inf)], (0,) * 8 + (1024,)),
    "below_big": (9, [(4, _ALL, -2e300)], _MID),                                  # finite, below the sentinel
    "accum": (9, [(slice(2, 6), _ALL, -3.5e299)], _MID),                          # no row below -1e300: the running score passes it at row 4
    "half_neginf": (9, [(4, _EVEN, -np.inf)], (0, 0, 0, 0, 512, 64, 0, 0, 0)),
    "one_alive": (9, [(4, _ALL, -np.inf), (4, 5, -3.0)], (0, 0, 0, 0, 1023, 939, 0, 0, 0)),
    # live scores of -9.9e299 absorb every later addend: all live states tie exactly for the rest of the table
    "straddle": (9, [(4, _EVEN, -1.5e300), (4, _ODD, -9.9e299)], (0, 0, 0, 0, 512, 64, 0, 0, 0)),
    "T1_neginf": (1, [(0, _ALL, -np.inf)], (1024,)),
}
FULLY_DEAD = ("neginf_mid", "neginf_first", "neginf_last", "below_big", "accum")       # deterministic decode refused
FIRST_DEAD = {"neginf_mid": 4, "neginf_first": 0, "neginf_last": 8, "below_big": 4, "accum": 4}   # the kept position the refusal names
PARTLY_DEAD = ("half_neginf", "one_alive", "straddle")                                 # a path exists
SWEEP_T = 17                            # an all -inf row at every index of random_rows(17, 7): each phase of the 4 + 4 unrolled loop
UNREACHABLE = "no state is reachable at kept position %d "
# deviate seeds of the nkeep = 16 runs: test_viterbi_tables.py asserts that none of these puts a deviate within 2^-40 of a boundary
DEAD_SEED = {"half_neginf": 41, "one_alive": 42}


def dead_rows(name):
    T, changes, _ = DEAD_CASES[name]
    rows = random_rows(*DEAD_BASE)[:T].copy()
    for r, s, v in changes:
        rows[r, s] = v
    return rows


def dead_batch():
    """(rows, deviates for nkeep = 16) of R = 3: a region that dies at row 4, one without positions, a live one"""
    rows = [dead_rows("neginf_mid"), random_rows(0, 32), random_rows(17, 33)]
    return rows, [deviates(16, 9, 31), np.zeros((16, 0)), deviates(16, 17, 33)]


def sweep_rows(at):
    rows = random_rows(SWEEP_T, 7)
    rows[at] = -np.inf
    return rows


def dead_counts(bp):
    return tuple(int(n) for n in np.count_nonzero(np.asarray(bp) == -1, axis=1))


def run_ld_until_dead(rows, skip, stay):
    """(long-double forward rows before the first whose total is 0, that row's index or T): from there the reference normalises
    0 / 0 and carries NaN"""
    f = np.asarray(V.start()[1], dtype=V.LD)
    out = []
    for t, o in enumerate(rows):
        with np.errstate(all="ignore"):
            f = V.step_ld(f, o, skip, stay)
        if not np.all(np.isfinite(f)):
            return np.array(out, dtype=V.LD).reshape(len(out), NS), t
        out.append(f)
    return np.array(out, dtype=V.LD).reshape(len(out), NS), len(rows)


def refused_steps(api, rows_list, region, position):
    """the deterministic decode of these rows is refused, naming the hook, the region and the kept position"""
    import pytest
    from poreseq_amd._capi import PoreseqError
    with pytest.raises(PoreseqError) as err:
        api.debug_viterbi_steps(rows_list, None, 0, SKIP, STAY, MMIN, MMAX)
    msg = str(err.value)
    assert "(-1)" in msg and "ps_debug_viterbi_steps: region %d: " % region in msg and UNREACHABLE % position in msg, msg


def deviates(nkeep, T, seed):
    """[nkeep][T] on the generator's 2^-31 grid, with the grid's two ends at a few back-steps"""
    r = np.random.default_rng(seed).integers(0, 2 ** 31, (nkeep, T)).astype(np.float64) / 2.0 ** 31
    for k in range(nkeep):
        r[k, (3 * k + 1) % T] = 0.0
        r[k, (5 * k + 2) % T] = (2.0 ** 31 - 1) / 2.0 ** 31
    return r


def attens(nkeep):
    return [MMIN + (MMAX - MMIN) * k / float(nkeep) for k in range(nkeep)]


TRACE_CASES = ((1, 33, 901), (16, 33, 902), (16, 9, 903))     # (nkeep, T, seed of rows and deviates)


def check_back_steps(paths, ref, rnd, nkeep, min_margin=None):
    """Every back-step on its own: given the path's state at position i, its state at i - 1 must be the one the deviate picks from
    the long-double weights.  With min_margin, also require that no deviate lies closer than that to an interior boundary."""
    T = ref.shape[0]
    bad, closest = [], 1.0
    for k, at in enumerate(attens(nkeep)):
        for i in range(T - 1, 0, -1):
            cum = V.pick_ld(ref[i], int(paths[k][i]), at, SKIP, STAY)
            want, margin = V.pick(cum, rnd[k][T - 1 - i])
            closest = min(closest, margin)
            if want != int(paths[k][i - 1]):
                bad.append((k, i, want, int(paths[k][i - 1])))
    if min_margin is not None:
        assert closest >= min_margin, "a deviate lies within %g of a boundary: pick another seed" % closest
    return bad


# ---- regions for the handle hook: (L, E, seed); holes in ref_align make the events contributing to a position span 1 .. E
REGIONS = ((90, 1, 611), (110, 2, 612), (100, 3, 613), (120, 4, 614), (130, 5, 615), (200, 8, 616))
DEEP_REGION = (60, 80, 617)            # more events than k_vit_obs_lds (72) and k_vit_obs<64> take
BATCH = ((100, 3, 613), (200, 8, 616), (90, 1, 611))
_regions = {}


def region(L, E, seed):
    """(draft, events) with staggered holes: event k keeps only the levels aligned before position L (E - k) / (E + 1) ... so the
    number of events with a level at a position falls from E to 1 along the region"""
    key = (L, E, seed)
    if key not in _regions:
        draft, events, _ = synth.make_region(L, E, seed, B.oracle_swalign, P0)
        events = copy.deepcopy(events)
        if E <= 8:
            for k, e in enumerate(events[1:], start=1):
                e.ref_align[e.ref_align > L * (E - k) / (E + 1.0)] = 0
        _regions[key] = (draft, events)
    draft, events = _regions[key]
    return draft, copy.deepcopy(events)


def contributing(events, L):
    """events with a level aligned to each position (the count the trimmed mean sees, up to the reference's index bookkeeping)"""
    n = np.zeros(L + 8, dtype=np.int64)
    for e in events:
        at = np.unique(e.ref_align[e.ref_align > 0].astype(np.int64))
        n[at[at < n.size]] += 1
    return n


def admitted_builds(E):
    """emission builds of the HIP library that take E events: k_vit_obs_lds, k_vit_obs<64>, k_vit_obs<256>"""
    return [b for b, cap in ((1, 72), (2, 64), (3, 256)) if E <= cap]


_oracle_tables = {}


def oracle_region_tables(key, nkeep):
    """the oracle's tables of a region (computed once per session)"""
    if (key, nkeep) not in _oracle_tables:
        draft, events = region(*key)
        orc = B.oracle_api()
        B.reset_rand()
        h = orc.align_create(draft, events, P0)
        try:
            _oracle_tables[(key, nkeep)] = orc.debug_viterbi([h], len(draft) + 64, nkeep, SKIP, STAY, MMIN, MMAX)[0]
        finally:
            orc.align_destroy(h)
    return _oracle_tables[(key, nkeep)]
