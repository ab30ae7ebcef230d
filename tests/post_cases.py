"""The cases of ps_posterior_stats (the sum over all alignments in an event's band and the expected moves under it), shared by
test_posterior.py (the restatement util.posterior_from_emissions against an explicit enumeration of paths and against the oracle's
max-plus tables, on the CPU) and test_hip_posterior.py (k_post_fwd / k_post_bwd on the GPU against that restatement).

  brute force         every lattice of n0 <= 4 levels and C <= 3 columns: every band per column (overlapping the previous one, apart
                      from it, below it), at most one column without a state; all paths enumerated one by one
  move_cases' cases   narrow, wide, untouched, empty_read, column0, all_unaligned, single, stay_run, poor — what each is there for is
                      said there
  n_column            narrow's draft with one base replaced by N.  populateStates (cpp/Sequence.h:84-98, sic) marks ONE state invalid
                      for it — the 5-mer the N leaves through — so this is one column without a state in the middle of every band
  n_run               the same draft with five consecutive N: five columns without a state next to each other

Everything derived from a case (the oracle's tables, the lattice, the restatements) is computed once and handed out unchanged."""
import copy
import itertools
import math

import numpy as np

import backends as B
import move_cases as M
import ref_cases
from poreseq_amd import util

LD = np.longdouble
EPS = 2.0 ** -52
COUNTS = ("e_skip", "e_match", "e_ignore", "e_insert", "e_stay", "e_extend")
MOVE_NAMES = tuple(n for n in M.NAMES if n != "mean_nan")      # (an AlignData marked non-finite is refused: a test of its own)
N_COLUMN, N_RUN = "n_column", "n_run"
NAMES = MOVE_NAMES + (N_COLUMN, N_RUN)
_made = {}


def _n_column(count):
    draft, events, par = M.case("narrow")
    at = len(draft) // 2
    assert "N" not in draft
    return draft[:at] + "N" * count + draft[at + count:], events, par


def case(name):
    """(draft, events, params); the caller owns the copies"""
    if name not in (N_COLUMN, N_RUN):
        return M.case(name)
    if name not in _made:
        _made[name] = _n_column(1 if name == N_COLUMN else 5)
    d, e, p = _made[name]
    return d, copy.deepcopy(e), dict(p)


def liks(ev):
    """the four log transition probabilities of an event as the library forms them (libm log of the model's prob_*)"""
    return tuple(math.log(float(getattr(ev.model, "prob_" + r))) for r in ("skip", "stay", "extend", "insert"))


def oracle_tables(name, e):
    """(main, stay) of the oracle's forward debug_fill of event e: the max-plus tables, NaN outside the band"""
    def make():
        draft, events, par = case(name)
        main, stay, _, _ = ref_cases.fill_tables(B.oracle_api(), draft, events, par, e, 0)
        return main, stay
    return ref_cases.once(("post_tables", name, e), make)


def lattice(name, e):
    """(obs, mask, valid, liks, n0, C) of event e of a case: the emissions of util.fill_emissions, the band of the oracle's tables"""
    def make():
        draft, events, par = case(name)
        states = B.oracle_api().seq_to_states(draft)
        main, _ = oracle_tables(name, e)
        return (util.fill_emissions(events[e], states, par), ~np.isnan(main), np.concatenate([[False], np.asarray(states) >= 0]),
                liks(events[e]), events[e].mean.size, len(states))
    return ref_cases.once(("post_lattice", name, e), make)


def restated(name, e, semiring="sum", dtype=np.float64):
    """util.posterior_from_emissions of event e of a case, with the per-level arrays (sum mode)"""
    def make():
        obs, mask, valid, lk, _, _ = lattice(name, e)
        return util.posterior_from_emissions(obs, mask, valid, *lk, semiring=semiring, dtype=dtype, levels=semiring == "sum")
    return ref_cases.once(("post_restated", name, e, semiring, np.dtype(dtype).name), make)


def n_events(name):
    return len(case(name)[1])


def inert(name, e):
    """ps_move_stats' rule: realign_width 0, no aligned level, or no level at all"""
    _, events, par = case(name)
    ev = events[e]
    with np.errstate(invalid="ignore"):
        return int(par["realign_width"]) == 0 or ev.mean.size == 0 or not bool(np.any(ev.ref_align > 0))


def rel_err(got, want, scale_floor=1.0):
    """|got - want| / max(scale_floor, |want|) elementwise in longdouble; equal infinities and NaN on both sides count as 0"""
    g, w = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - w) / np.maximum(LD(scale_floor), np.abs(w))
    same = (g == w) | (np.isnan(g) & np.isnan(w))
    return np.where(same, LD(0), err)


# ---- brute force: every path of a small lattice, one by one ---------------------------------------------------------------------------
def small_lattices(max_n0=4, max_C=3):
    """(n0, bands, valid): every choice of one band (i0, i1) per column — whatever the previous column's — with all columns valid
    or exactly one not"""
    for n0 in range(1, max_n0 + 1):
        rows = [(a, b) for a in range(1, n0 + 1) for b in range(a, n0 + 1)]
        for C in range(1, max_C + 1):
            for bands in itertools.product(rows, repeat=C):
                for dead in [None] + list(range(C)):
                    yield n0, bands, tuple(k != dead for k in range(C))


def small_arrays(n0, bands, valid, rng):
    """(obs, mask, valid array) of a small lattice, emissions drawn between -4 and 3"""
    C = len(bands)
    mask = np.zeros((n0 + 1, C + 1), dtype=bool)
    mask[:, 0] = True
    for j, (a, b) in enumerate(bands, 1):
        mask[a:b + 1, j] = True
    return rng.uniform(-4.0, 3.0, (n0 + 1, C + 1)), mask, np.array((False,) + tuple(valid))


def enumerate_paths(n0, bands, valid, obs, lk):
    """logz and the six expected counts of a small lattice in longdouble, from the list of ALL paths: the text of
    include/poreseq_hip.h read as a grammar of paths, scalar code that shares nothing with the restatement.  A path is a start —
    a floor term, or a move out of a constant / implicit cell — a run of moves, and an end in a main cell."""
    lsk, lst, lex, lin = (LD(v) for v in lk)
    C = len(bands)
    band = lambda j: (0, n0) if j == 0 else bands[j - 1]
    live = lambda j: j >= 1 and valid[j - 1]
    o = lambda i, j: LD(obs[i, j])

    def ext(paths, w, move):
        for pw, pc in paths:
            c = dict(pc)
            c[move] = c.get(move, 0) + 1
            yield pw + w, c

    def into_main(i, j):
        i0, _ = band(j)
        p0, p1 = band(j - 1)
        yield LD(0), {}
        if p0 <= i <= p1 and live(j - 1):
            yield from ext(into_main(i, j - 1), lsk, "e_skip")
        else:
            yield lsk, {"e_skip": 1}
        if p0 < i <= p1:
            if live(j - 1):
                yield from ext(into_main(i - 1, j - 1), o(i, j), "e_match")
                yield from ext(into_main(i - 1, j - 1), lin, "e_ignore")
            else:
                yield o(i, j), {"e_match": 1}
                yield lin, {"e_ignore": 1}
        else:
            yield o(i, j), {"e_match": 1}
        if i > i0:
            yield from ext(into_main(i - 1, j), lin, "e_insert")
            yield from into_stay(i, j)

    def into_stay(i, j):
        i0, _ = band(j)
        if i <= i0:
            return
        yield LD(0), {}
        yield from ext(into_main(i - 1, j), o(i, j) + lst, "e_stay")
        yield from ext(into_stay(i - 1, j), o(i, j) + lex, "e_extend")

    paths = []
    for j in range(1, C + 1):
        if live(j):
            for i in range(bands[j - 1][0], bands[j - 1][1] + 1):
                paths.extend(into_main(i, j))
    if not paths:
        return LD(0), dict.fromkeys(COUNTS, LD(0)), 0
    w = np.array([p[0] for p in paths], dtype=LD)
    top = np.max(w)
    logz = top + np.log(np.sum(np.exp(w - top)))
    post = np.exp(w - logz)
    counts = {k: np.sum(post * np.array([p[1].get(k, 0) for p in paths], dtype=LD)) for k in COUNTS}
    return logz, counts, len(paths)
