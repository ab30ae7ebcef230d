"""The HIP path against the oracle over a lattice of parameters (tests/sweep_cases.py, which test_sweep.py holds to the live
reference build) and Smith-Waterman on bytes outside ACGT.  Everything is compared at tolerance 0.

Parameters: 24 random small regions x {sweep, sweep_w2, sweep_w4, fill} — scoring bands of 0, 1, 2 and up to 511, bands several
times wider than the realign band, point widths 0 .. 60, random transition probabilities, alignments with holes and jumps, an
event that never aligned, edits in every size class of k_score — and three 1300-base cases whose edits of 59 .. 130 inserted bases
meet a scoring band of 511 (k_score<64>'s chunk carry over all 1023 rows).  The oracle's answers are computed once per seed and
shared between the families.  conftest.py fans only two modules over the families, so this one asks for them itself.

Smith-Waterman: alphabets with N, lower case, every byte 1 .. 127 and the NUL byte, on lengths that leave padded columns behind
n2, under every fill (4 / 8 / 16 columns per lane, the packed 16-bit fill, one workgroup per pair, the band fill) and all three
traceback forms (index lists, summaries, the map build of ScoreSequences); launch counters say which fill ran.  The packed fill's
length limit is pinned at 13 000 / 13 001.

A lattice value that the library refuses is a finding, not a reason to skip: none is skipped or xfailed here."""
import copy
import os

import numpy as np
import pytest

import backends as B
import sweep_cases as S
import tiled_cases as TC
from poreseq_amd import _capi, synth
from poreseq_amd.poreseqcpp import PSAlign
from poreseq_amd.util import DEFAULT_PARAMS

pytestmark = pytest.mark.gpu
FILLS = ["sweep", "sweep_w2", "sweep_w4", "fill"]
families = pytest.mark.parametrize("fwd_kernel", FILLS, indirect=True)      # topmost decorator: the family varies fastest


class Counters:
    """launch counters of the library while the block runs"""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        self.api = _capi.load_hip()
        self.api.prof_enable(1)
        self.api.prof_reset()
        return self

    def __exit__(self, *exc):
        self.n = {k: self.api.prof_get(k)[1] for k in self.names}
        self.api.prof_enable(0)
        return False


# ---- the lattice ----------------------------------------------------------------------------------------------------------------
def oracle_log(seed):
    return TC.oracle_once(("sweep", seed), lambda: S.full_log(B.OraclePSAlign, seed))


@families
@pytest.mark.parametrize("seed", S.SEEDS)
def test_every_call_equals_the_oracle(seed, fwd_kernel):
    """ScoreEvents, ScorePoints, ScoreMutations, Mutate(reps=2), Refine with the sequences and every event's refs after them on one
    object, Mutate('viterbi', 1) on the events as generated and on the holed ones"""
    want = oracle_log(seed)
    got = S.full_log(PSAlign, seed)
    for k in want:
        if got[k] != want[k] and k in ("ScorePoints", "ScoreMutations"):
            bad = [(i, x, y) for i, (x, y) in enumerate(zip(got[k], want[k])) if x != y]
            raise AssertionError("%s: %d of %d edits differ, first %r" % (k, len(bad), len(want[k]), bad[:3]))
        assert got[k] == want[k], k


@families
@pytest.mark.parametrize("seed", S.SEEDS)
def test_dp_matrices_of_one_event(seed, fwd_kernel):
    """forward and backward main / stay matrices and the forward step codes of the first event (holes and jumps included)"""
    draft, holed, clean, P, muts = S.case(seed)
    hip = _capi.load_hip()
    for d in (0, 1):
        want = TC.oracle_once(("sweep_dp", seed, d), lambda: TC.fill_tables(B.oracle_api(), draft, holed, P, 0, d))
        got = TC.fill_tables(hip, draft, holed, P, 0, d)
        for k, (x, y) in enumerate(zip(got, want)):
            if d == 1 and k >= 2:
                continue   # backward step codes are not kept (nothing reads them)
            if not np.array_equal(x, y, equal_nan=True):
                differs = ~((x == y) | (np.isnan(x.astype(np.float64)) & np.isnan(y.astype(np.float64))))
                cols = np.flatnonzero(differs.any(axis=0))
                raise AssertionError("direction %d, table %d: first differing column %d (rows %s), %d cells differ"
                                     % (d, k, cols[0], np.flatnonzero(differs[:, cols[0]])[:8].tolist(), int(differs.sum())))


@families
def test_the_family_asked_for_ran_on_the_lattice(fwd_kernel):
    """the fixture's choice reaches these cases: on some seed the family's kernel ran and the other family's did not (the library
    steps down to fewer wavefronts, or to k_fill, where no strip form fits a band)"""
    hip = _capi.load_hip()
    seen = []
    for seed in S.SEEDS[:8]:
        draft, holed, clean, P, muts = S.case(seed)
        with Counters("sweep", "fill", "sweep_w2", "sweep_w4") as c:
            B.make_pa(PSAlign, draft, copy.deepcopy(clean), P).ScoreEvents()
        seen.append(c.n)
        alone = c.n["fill"] > 0 and c.n["sweep"] == 0 if fwd_kernel == "fill" else c.n["sweep"] > 0 and c.n["fill"] == 0 and c.n.get(fwd_kernel, 1) > 0
        if alone:
            return
    raise AssertionError((fwd_kernel, seen))


@pytest.mark.parametrize("seed", S.SEEDS)
def test_point_table_support_and_score_sequences(seed):
    """the library's own choice of kernels: PointTable, ScoreMutationSupport, ScoreSequences of three corrupted copies of the draft"""
    want = TC.oracle_once(("sweep_own", seed), lambda: S.own_choice_log(B.OraclePSAlign, seed))
    got = S.own_choice_log(PSAlign, seed)
    assert S.same_own_choice(got, want)


@families
@pytest.mark.parametrize("k", range(len(S.DIRECTED_WIDTHS)))
def test_long_edits_against_a_wide_scoring_band(k, fwd_kernel):
    draft, events, P, muts = S.directed(k)
    want = TC.oracle_once(("directed", k), lambda: S.listing(B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P).ScoreMutations(muts)))
    with Counters("score_g64") as c:
        got = S.listing(B.make_pa(PSAlign, draft, copy.deepcopy(events), P).ScoreMutations(muts))
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(got, want)) if x != y]
    assert not bad, bad[:3]
    assert c.n["score_g64"] > 0


def test_every_size_class_of_k_score_runs_on_the_lattice():
    """over the 24 seeds together each of k_score's five builds is launched (host-side counters), with the results the oracle's"""
    total = {k: 0 for k in S.SCORE_CLASSES}
    for seed in S.SEEDS:
        draft, holed, clean, P, muts = S.case(seed)
        with Counters(*S.SCORE_CLASSES) as c:
            got = S.listing(B.make_pa(PSAlign, draft, copy.deepcopy(holed), P).ScoreMutations(muts))
        assert got == oracle_log(seed)["ScoreMutations"], seed
        for k in total:
            total[k] += c.n[k]
    assert all(v > 0 for v in total.values()), total


# ---- Smith-Waterman on bytes outside ACGT ---------------------------------------------------------------------------------------
ALPHABETS = {"ACGTN": "ACGTN", "mixed_case": "ACGTacgtN-", "bytes_1_127": "".join(chr(c) for c in range(1, 128)), "nul": "AC\x00"}
LENGTHS = [(1, 1), (63, 65), (130, 120), (700, 640), (600, 2049)]
OFF = dict(PORESEQ_SW_BAND="off")
# name -> (environment, counter that must be > 0, counter that must be 0)
SW_FILLS = {
    "k4": (dict(OFF, PORESEQ_SW_K="4"), None, "sw_pk8"),
    "k8_packed": (dict(OFF, PORESEQ_SW_K="8"), "sw_pk8", "sw_band"),
    "k8_32bit": (dict(OFF, PORESEQ_SW_K="8", PORESEQ_SW_PK="0"), None, "sw_pk8"),
    "k16": (dict(OFF, PORESEQ_SW_K="16"), None, "sw_pk8"),
    "one_workgroup": (dict(OFF, PORESEQ_SW_FORM="one"), None, "sw_pk8"),
    "band": (dict(PORESEQ_SW_BAND="force", PORESEQ_SW_BAND_W="128", PORESEQ_SW_K="8"), "sw_band", None),
}
SW_ENV = ("PORESEQ_SW_BAND", "PORESEQ_SW_BAND_W", "PORESEQ_SW_K", "PORESEQ_SW_PK", "PORESEQ_SW_FORM")


class sw_env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SW_ENV}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in SW_ENV:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


def sw_pairs(alphabet):
    """s2 is s1 with every ninth byte redrawn, cut to n2 or continued by a random tail; n2 off a multiple of the lane span"""
    letters = ALPHABETS[alphabet]
    rng = np.random.default_rng(sorted(ALPHABETS).index(alphabet) + 31)
    draw = lambda n: [letters[i] for i in rng.integers(0, len(letters), n)]   # (not a numpy string array: it would drop the NUL)
    out = []
    for n1, n2 in LENGTHS:
        a = draw(n1)
        b = list(a)
        b[::9] = draw(len(b[::9]))
        b = b[:n2] if n2 <= n1 else b + draw(n2 - n1)
        out.append(("".join(a), "".join(b)))
    return out


def sw_oracle(alphabet):
    def make():
        pairs = sw_pairs(alphabet)
        return [B.oracle_api().swfull(a, b) for a, b in pairs], B.oracle_api().sw_summaries(pairs)
    return TC.oracle_once(("sw", alphabet), make)


def same_float(x, y):
    return x == y or (np.isnan(x) and np.isnan(y))


@pytest.mark.parametrize("fill", list(SW_FILLS))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_smith_waterman_on_any_byte(alphabet, fill):
    """index lists (swfull) and summaries (one batch) of the five pairs against the oracle, whose comparison is the reference's:
    bytes are equal or not (cpp/swlib.cpp:260).  The NUL alphabet failed before the padded columns got a code no byte can have:
    a NUL in seq1 matched the padding, and the maximum could lie outside the matrix."""
    env, must_run, must_not = SW_FILLS[fill]
    pairs = sw_pairs(alphabet)
    want_lists, want_sums = sw_oracle(alphabet)
    hip = _capi.load_hip()
    with sw_env(env), Counters("sw_pk8", "sw_band", "sw_lists", "sw_summary") as c:
        got_lists = [hip.swfull(a, b) for a, b in pairs]
        got_sums = hip.sw_summaries(pairs)
    assert c.n["sw_lists"] >= len(pairs) and c.n["sw_summary"] >= 1
    if must_run:
        assert c.n[must_run] > 0, c.n
    if must_not:
        assert c.n[must_not] == 0, c.n
    for (n1, n2), g, w in zip(LENGTHS, got_lists, want_lists):
        assert g[0] == w[0] and same_float(g[1], w[1]), ((n1, n2), g[:2], w[:2])
        assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), (n1, n2)
    for (n1, n2), g, w in zip(LENGTHS, got_sums, want_sums):
        assert tuple(g)[:-1] == tuple(w)[:-1] and same_float(g.accuracy, w.accuracy), ((n1, n2), g, w)


@pytest.mark.parametrize("fill", ["k4", "k8_packed", "band"])
def test_score_sequences_of_candidates_with_n_and_lower_case(fill):
    """the map build of the traceback (ScoreSequences) on candidate sequences holding N and lower-case bases, against the literal
    loop `RealignTo; ScoreEvents` on the oracle"""
    P = dict(DEFAULT_PARAMS, verbose=0)
    draft, events, _ = synth.make_region(333, 3, 4711, B.oracle_swalign, P)
    rng = np.random.default_rng(4711)
    cands = []
    for rate in (0.02, 0.05):
        s = np.array(list(synth.corrupt(rng, draft, rate, rate, rate)))
        k = rng.choice(s.size, 12, replace=False)
        s[k[:6]] = "N"
        s[k[6:]] = np.char.lower(s[k[6:]])
        cands.append("".join(s))
    want = TC.oracle_once(("sw_map",), lambda: B.make_pa(B.OraclePSAlign, draft, copy.deepcopy(events), P).ScoreSequences(cands))
    env, must_run, must_not = SW_FILLS[fill]
    with sw_env(env), Counters("sw_pk8", "sw_band", "sw_map") as c:
        got = B.make_pa(PSAlign, draft, copy.deepcopy(events), P).ScoreSequences(cands)
    assert c.n["sw_map"] > 0 and (not must_run or c.n[must_run] > 0) and (not must_not or c.n[must_not] == 0), c.n
    assert got.shape == (2, len(events)) and np.array_equal(got, want)


def test_packed_fill_length_limit():
    """scores reach 5 x min(n1, n2): an identical pair of 13 000 bases (65 000) still takes the packed 16-bit fill, 13 001 bases the
    32-bit one; the expected values follow from the sequences being identical"""
    rng = np.random.default_rng(13)
    s = synth.random_sequence(rng, 13001)
    hip = _capi.load_hip()
    for n, packed in ((13000, True), (13001, False)):
        with sw_env(dict(OFF, PORESEQ_SW_K="8")), Counters("sw_pk8") as c:
            score, acc, i1, i2 = hip.swfull(s[:n], s[:n])
        assert (c.n["sw_pk8"] > 0) == packed, (n, c.n)
        assert score == 5 * n and acc == 100.0
        assert np.array_equal(i1, np.arange(1, n + 1)) and np.array_equal(i2, i1)
    t = synth.random_sequence(rng, 700)
    for env in (dict(OFF, PORESEQ_SW_K="8"), dict(PORESEQ_SW_K="8")):   # one batch of both and a short pair: full matrices, then the library's band choice
        with sw_env(env):
            got = hip.sw_summaries([(s[:13000], s[:13000]), (s, s), (t, t)])
        for n, g in zip((13000, 13001, 700), got):
            assert tuple(g) == (5 * n, n, n, 1, 1, n, n, 0, 0, 100.0), (n, g)
