"""Random small regions over a lattice of parameter values, shared by test_sweep.py (the oracle against the live reference build)
and test_hip_sweep.py (the HIP path against the oracle), so that neither side depends on which parameter sets someone thought of.

`case(seed, swalign)` is the generator of test_oracle.py's random sweep — alignments with a hole, a forward jump, an event that
never aligned, random multi-base edits at both ends of the sequence and past its end — drawing from a wider lattice: scoring bands
of 0, 1 and 2 and bands several times wider than the realign band, point widths of 0, 1, 2 and 60, random transition probabilities
and inserted lengths on either side of every size class of the edit-scoring kernel (columns = inserted + 6: up to 7, 8, 16, 32,
more; 59 / 60 / 61 inserted bases straddle the 64-column chunk of the last class).  All of it lies inside the library's documented
limits (realign_width <= 1022, scoring_width <= 511 with edits over 58 bases, <= 256 events).

`directed(k, swalign)` are three long two-event regions whose edits of 59 .. 130 inserted bases meet a scoring band of 511 (or
300): with about 1100 levels the carried column of the 64-column chunks spans all 1023 rows.

test_oracle.py's own sweep keeps its seeds, lattice and assertions; this module does not touch synth's seeded streams."""
import copy

import numpy as np

import backends as B
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS, MutationInfo

SEEDS = list(range(100, 124))
REALIGN = (3, 7, 20, 45, 64, 129, 300)
SCORING = (0, 1, 2, 9, 30, 100, 300, 511)
POINT = (0, 1, 2, 5, 20, 60)
OFFSET = (0.0, 0.5, 4.5, 12.0)
TRANS = (0.005, 0.02, 0.1, 0.3)
INSERTED = (0, 1, 2, 5, 8, 20, 30, 59, 60, 61, 70)   # 20: the only length whose columns (26) fall in the 17 .. 32 class
TRANS_KEYS = tuple(k + s for k in ("skip", "stay", "extend", "insert") for s in ("_t", "_c"))
SCORE_CLASSES = ("score_g7", "score_g8", "score_g16", "score_g32", "score_g64")

DIRECTED_WIDTHS = ((300, 511), (120, 511), (300, 300))   # (realign_width, scoring_width)


def edit(start, orig, mut):
    mi = MutationInfo()
    mi.start, mi.orig, mi.mut = int(start), orig, mut
    return mi


def punch(rng, events, draft_len):
    """a copy of the events with a hole, a forward jump and (sometimes) a last event that never aligned"""
    ev = copy.deepcopy(events)
    E = len(ev)
    for k, e in enumerate(ev):
        n = e.ref_align.size
        if n > 60 and rng.random() < 0.6:
            a, b = sorted(rng.integers(5, n - 5, 2))
            e.ref_align[a:b] = 0                                               # a hole
        if n > 80 and rng.random() < 0.5:
            c = int(rng.integers(10, n - 50))
            e.ref_align[c:c + 30] = np.minimum(e.ref_align[c:c + 30] + 40, draft_len - 5) * (e.ref_align[c:c + 30] > 0)   # a jump
        if E > 1 and k == E - 1 and rng.random() < 0.3:
            e.ref_align[:] = 0                                                 # an event that never aligned
    return ev


def _columns():
    """one value per seed for each of the four width / offset parameters: every lattice value at least three times over the 24
    seeds, each parameter's column in an order of its own (so the combinations are random and no value depends on a lucky draw)"""
    rng = np.random.default_rng(20240)
    cols = {}
    for name, values in (("realign_width", REALIGN), ("scoring_width", SCORING), ("point_width", POINT), ("lik_offset", OFFSET)):
        col = (list(values) * len(SEEDS))[:len(SEEDS)]
        cols[name] = [float(col[k]) for k in rng.permutation(len(SEEDS))]
    return cols


_COLUMNS = _columns()
_cases = {}


def case(seed, swalign=None):
    """(draft, events with holes, events as generated, params, edits) of one seed; the same objects on every call — copy the events
    before handing them to a backend"""
    swalign = B.oracle_swalign if swalign is None else swalign
    key = ("case", seed, swalign)
    if key not in _cases:
        rng = np.random.default_rng(seed)
        P = dict(DEFAULT_PARAMS, verbose=0, **{k: col[SEEDS.index(seed)] for k, col in _COLUMNS.items()})
        for k in TRANS_KEYS:
            P[k] = float(rng.choice(TRANS))
        L, E = int(rng.integers(60, 320)), int(rng.integers(1, 9))
        draft, events, _ = synth.make_region(L, E, 900 + seed, swalign, P)
        holed = punch(rng, events, len(draft))
        muts = synth.random_point_mutations(rng, draft, 25)
        for _ in range(12):
            st = int(rng.integers(0, len(draft) + 2))
            no, nm = int(rng.integers(0, 6)), int(rng.choice(INSERTED))
            if no or nm:
                muts.append(edit(st, draft[st:st + no], "".join(rng.choice(list("ACGT"), nm))))
        _cases[key] = (draft, holed, events, P, muts)
    return _cases[key]


def directed(k, swalign=None):
    """(draft, events, params, edits) of the k-th long case: edits over 58 bases against a wide scoring band"""
    swalign = B.oracle_swalign if swalign is None else swalign
    key = ("directed", k, swalign)
    if key not in _cases:
        W, SW = DIRECTED_WIDTHS[k]
        P = dict(DEFAULT_PARAMS, verbose=0, realign_width=float(W), scoring_width=float(SW))
        draft, events, _ = synth.make_region(1300, 2, 7700 + k, swalign, P)
        rng = np.random.default_rng(7700 + k)
        n = len(draft)
        ins = lambda m: "".join(rng.choice(list("ACGT"), m))
        spec = [(600, 0, 59), (640, 2, 60), (700, 0, 61), (30, 1, 70), (n - 20, 3, 64), (650, 5, 130), (655, 70, 0), (2, 0, 65)]
        muts = [edit(st, draft[st:st + no], ins(nm)) for st, no, nm in spec]
        _cases[key] = (draft, events, P, muts)
    return _cases[key]


def score_class(draft_len, width, mi):
    """the size class of the edit-scoring kernel an edit falls in (columns = inserted + 6, cut at the end of the edited sequence;
    none with a scoring band of 0 or a start past the end), or None when nothing is scored for it"""
    L = draft_len
    if int(width) == 0 or mi.start > L:
        return None
    cut = min(L, mi.start + len(mi.orig))
    Lm = L if mi.start >= L else mi.start + len(mi.mut) + (L - cut)
    Cm = Lm - 4 if Lm >= 5 else 0
    ncol = min(len(mi.mut) + 6, max(0, Cm - max(mi.start - 4, 0)))
    return SCORE_CLASSES[0 if ncol <= 7 else 1 if ncol <= 8 else 2 if ncol <= 16 else 3 if ncol <= 32 else 4]


def listing(scored):
    return [(s.start, s.orig, s.mut, s.score) for s in scored]


def refs(pa):
    return [e.ref_align.tolist() for e in pa.events], [e.ref_like.tolist() for e in pa.events]


def candidates(draft, seed):
    """three corrupted copies of the draft for ScoreSequences"""
    rng = np.random.default_rng(5000 + seed)
    return [synth.corrupt(rng, draft, 0.02, 0.02, 0.02), synth.corrupt(rng, draft, 0.05, 0.05, 0.05), synth.corrupt(rng, draft[8:-8], 0.01, 0.01, 0.01)]


def full_log(cls, seed, swalign=None, holed_viterbi=True):
    """every API result of one backend on a seed's case, by name.  The first block runs on ONE object, call after call, as the sweep
    of test_oracle.py does; ViterbiMutate runs on the events as generated and (holed_viterbi: not for the reference's own code,
    which reads out of bounds there) on the holed ones."""
    draft, holed, clean, P, muts = case(seed, swalign)
    mk = lambda ev: B.make_pa(cls, draft, copy.deepcopy(ev), P)
    log = {}
    B.reset_rand()
    pa = mk(holed)
    log["ScoreEvents"] = pa.ScoreEvents()
    log["ScorePoints"] = listing(pa.ScorePoints())
    log["ScoreMutations"] = listing(pa.ScoreMutations(muts))
    log["Mutate"] = (pa.Mutate(reps=2), pa.sequence)
    log["Refine"] = (pa.Refine(), pa.sequence)
    log["refs"] = refs(pa)
    B.reset_rand()
    pv = mk(clean)
    log["viterbi"] = (pv.Mutate(seqs="viterbi", reps=1), pv.sequence, refs(pv))
    if holed_viterbi:
        B.reset_rand()
        pv = mk(holed)
        log["viterbi_holed"] = (pv.Mutate(seqs="viterbi", reps=1), pv.sequence, refs(pv))
    return log


def own_choice_log(cls, seed, swalign=None, support=True):
    """PointTable, ScoreMutationSupport and ScoreSequences of a seed's case (a library without the first and the last entry point
    runs the literal definitions in poreseqcpp.py; support=False for the reference build, which cannot give per-event terms)"""
    draft, holed, clean, P, muts = case(seed, swalign)
    mk = lambda ev: B.make_pa(cls, draft, copy.deepcopy(ev), P)
    tb = mk(holed).PointTable()
    sc, sup, lst = mk(holed).ScoreMutationSupport(muts) if support else (np.zeros(0), np.zeros(0), [])
    return {"PointTable": tb, "Support": (sc, sup, listing(lst)), "ScoreSequences": mk(clean).ScoreSequences(candidates(draft, seed))}


def same_own_choice(a, b):
    from point_cases import same
    return (same(a["PointTable"], b["PointTable"]) and np.array_equal(a["Support"][0], b["Support"][0]) and np.array_equal(a["Support"][1], b["Support"][1])
            and a["Support"][2] == b["Support"][2] and np.array_equal(a["ScoreSequences"], b["ScoreSequences"]))
