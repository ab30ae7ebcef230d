"""The yardstick of the phase of het edits (ps_score_mutation_phase), shared by test_phase.py (the fallback path on the CPU checkers)
and test_hip_phase.py (k_link, k_phase, k_haptag on the GPU): the definition restated as plain loops over (site, w, event), run over
the ORACLE's score_mutation_deltas and the ref_align the oracle's AlignData holds after that call (support_cases.oracle_terms).

  cover(e, m)         support_cases.covers
  link[m][w - 1]      the pair (m, j = m + w), w = 1 .. W, all zero where j >= M; for e ascending with cover(e, m) and cover(e, j),
                      da = delta[e][m], db = delta[e][j], s = da + db, r = da - db:
                        cis   += (s if s > 0 else 0.0) + log(0.5 + 0.5 exp(-|s|))
                        trans += (da if da > db else db) + log(0.5 + 0.5 exp(-|r|))
                        n_both += 1;  n_cis += both > 0 or both < 0;  n_trans += one > 0 and the other < 0
  phase[m]            site 0: vote 0.0, hap +1, set 0.  m > 0: vote = 0.0; for w = 1 .. min(W, m), i = m - w, L = link[i][w - 1]:
                      set[i] == set[m - 1] and L.n_both > 0  ->  vote += hap[i] * (L.cis - L.trans).  vote != 0 and |vote| >= min_link:
                      joins set[m - 1] with hap = +1 if vote > 0 else -1; otherwise set[m - 1] + 1 with hap +1.
  hap[e][k], k < S    lik1 / n1 over the sites m of set k with cover(e, m) and hap +1, lik2 / n2 with hap -1; partial l = 0.0 plus
                      delta[e][m] for m = l, l + 64, ... ascending, then the 64 partials into 0.0 for l = 0 .. 63.

`links` evaluates the records in float64 (numpy's exp and log on scalars, the functions util.phase_from_deltas calls) or in
numpy.longdouble (80-bit here, asserted by genotype_cases).  Counts and ints are compared for equality.  cis / trans are compared
with the long double loop under a DERIVED bound of the genotype bound's form:

  |got - ref| <= 2^-52 (16 + n_both) sum over the shared events of (1 + |da| + |db|)

Per term: one rounding of s or r (at most 2^-53 (|da| + |db|)), one ulp each from exp and log with |log x| <= 0.7 — an error of
2^-52 in exp(-|s|) <= 1 moves x in [0.5, 1] by 2^-53 and log x by at most 2^-52 — and one add of two numbers of at most |da| + |db|
+ 0.7: 16 * 2^-52 (1 + |da| + |db|) covers them with room; the in-order sum adds n_both roundings of a running total of at most
that sum.

The phase is held two ways.  (a) `replay`: the rule in float64 on the records the call ITSELF returned — vote byte for byte, ints
equal: this pins the scan whatever the last bits of cis / trans are.  (b) `decisions`: the scan on the long double links.  A
precondition, asserted: every site whose vote has at least one term has ||vote| - min_link| > 1e-6 and |vote| > 1e-6 there, seven
orders of magnitude above the bound, so no rounding of a correct evaluation can turn a decision.  A site whose vote has NO term (it
shares no covering event with any site of the set before it) has vote 0.0 exactly in every arithmetic and opens a set by the rule:
it is compared like the others.  No site is left out.

With the phase equal, lik1 / lik2 are byte for byte `tags`' lane-ordered float64 sums over the oracle's terms, and the scores are
byte for byte support_cases' sums."""
import numpy as np

import genotype_cases  # noqa: F401  (asserts that numpy.longdouble is the 80-bit format)
import support_cases as S
from poreseq_amd import _capi

MARGIN = 1e-6


def links(terms, L, W, real):
    """(cis [M][W], trans [M][W] as lists of `real`, counts int32 [M, W, 3]: n_both, n_cis, n_trans) by the definition"""
    starts, delta, spans = terms
    E, M = len(delta), len(starts)
    assert np.isfinite(np.array(delta, dtype=np.float64)).all()          # precondition: no case is left out of the comparison
    zero, half = real(0.0), real(0.5)
    cis = [[real(0.0) for _ in range(W)] for _ in range(M)]
    trans = [[real(0.0) for _ in range(W)] for _ in range(M)]
    cnt = np.zeros((M, W, 3), dtype=np.int32)
    for m in range(M):
        for w in range(1, W + 1):
            j = m + w
            if j >= M:
                continue
            c, t = real(0.0), real(0.0)
            for e in range(E):
                if not (S.covers(spans, starts, L, e, m) and S.covers(spans, starts, L, e, j)):
                    continue
                da, db = real(delta[e][m]), real(delta[e][j])
                s, r = da + db, da - db
                c = c + ((s if s > 0 else zero) + np.log(half + half * np.exp(-np.abs(s))))
                t = t + ((da if da > db else db) + np.log(half + half * np.exp(-np.abs(r))))
                cnt[m, w - 1, 0] += 1
                cnt[m, w - 1, 1] += (da > 0 and db > 0) or (da < 0 and db < 0)
                cnt[m, w - 1, 2] += (da > 0 and db < 0) or (da < 0 and db > 0)
            cis[m][w - 1], trans[m][w - 1] = c, t
    return cis, trans, cnt


def scan(cis, trans, n_both, W, min_link, real):
    """(votes [M] of `real`, hap [M], set [M], terms [M]: how many links entered each vote) by the rule"""
    M = len(cis)
    votes, hap, sets, nterm = [], [], [], []
    lim = real(min_link)
    for m in range(M):
        if m == 0:
            votes.append(real(0.0)); hap.append(1); sets.append(0); nterm.append(0)
            continue
        vote, n = real(0.0), 0
        for w in range(1, min(W, m) + 1):
            i = m - w
            if sets[i] == sets[m - 1] and n_both[i][w - 1] > 0:
                vote = vote + real(hap[i]) * (cis[i][w - 1] - trans[i][w - 1])
                n += 1
        if vote != 0 and np.abs(vote) >= lim:
            sets.append(sets[m - 1]); hap.append(1 if vote > 0 else -1)
        else:
            sets.append(sets[m - 1] + 1); hap.append(1)
        votes.append(vote); nterm.append(n)
    return votes, hap, sets, nterm


def replay(link, min_link):
    """_capi.EDIT_PHASE [M]: the rule in float64 on link records as a call returned them ((a) above)"""
    link = np.asarray(link)
    M, W = link.shape
    cis = [[np.float64(v) for v in row] for row in link["cis"].tolist()]
    trans = [[np.float64(v) for v in row] for row in link["trans"].tolist()]
    votes, hap, sets, _ = scan(cis, trans, link["n_both"].tolist(), W, min_link, np.float64)
    out = np.zeros(M, dtype=_capi.EDIT_PHASE)
    out["vote"], out["hap"], out["set"] = [float(v) for v in votes], hap, sets
    return out


def tags(terms, L, hap, sets, n_events, max_sets):
    """_capi.EVENT_HAP [E, S]: the lane-ordered float64 sums over the oracle's terms for the phase (hap [M], set [M])"""
    starts, delta, spans = terms
    M = len(starts)
    out = np.zeros((n_events, max_sets), dtype=_capi.EVENT_HAP)
    for e in range(n_events):
        for k in range(max_sets):
            for sign, lik, cnt in ((1, "lik1", "n1"), (-1, "lik2", "n2")):
                part, n = [0.0] * 64, 0
                for m in range(M):
                    if sets[m] == k and hap[m] == sign and S.covers(spans, starts, L, e, m):
                        part[m % 64] = part[m % 64] + delta[e][m]
                        n += 1
                tot = 0.0
                for lane in range(64):
                    tot = tot + part[lane]
                out[lik][e, k], out[cnt][e, k] = tot, n
    return out


def bound(terms, L, W):
    """float64 [M, W]: 2^-52 (16 + n_both) sum over the shared events of (1 + |da| + |db|)"""
    starts, delta, spans = terms
    M = len(starts)
    out = np.zeros((M, W))
    for m in range(M):
        for w in range(1, W + 1):
            j = m + w
            if j >= M:
                continue
            ds = [abs(delta[e][m]) + abs(delta[e][j]) for e in range(len(delta))
                  if S.covers(spans, starts, L, e, m) and S.covers(spans, starts, L, e, j)]
            out[m, w - 1] = 2.0 ** -52 * (16 + len(ds)) * sum(1.0 + d for d in ds)
    return out


def yardstick(terms, L, n_events, window, min_link, max_sets):
    """one case: the float64 records (link, phase, hap, n_sets), the long double cis / trans, the bound, the long double scan's
    decisions and the smallest margins of its votes"""
    W = int(window)
    starts = terms[0]
    M = len(starts)
    c64, t64, cnt = links(terms, L, W, np.float64)
    cld, tld, cnt2 = links(terms, L, W, np.longdouble)
    assert np.array_equal(cnt, cnt2)
    link = np.zeros((M, W), dtype=_capi.EDIT_LINK)
    if M:
        link["cis"], link["trans"] = np.array(c64, dtype=np.float64).reshape(M, W), np.array(t64, dtype=np.float64).reshape(M, W)
        link["n_both"], link["n_cis"], link["n_trans"] = cnt[:, :, 0], cnt[:, :, 1], cnt[:, :, 2]
    phase = replay(link, min_link) if M else np.zeros(0, dtype=_capi.EDIT_PHASE)
    vld, hld, sld, nterm = scan(cld, tld, cnt[:, :, 0].tolist(), W, min_link, np.longdouble)
    live = [abs(float(v)) for v, n in zip(vld, nterm) if n]
    return {
        "W": W, "min_link": float(min_link), "S": int(max_sets), "M": M, "E": n_events,
        "link": link, "phase": phase, "n_sets": (int(phase["set"][-1]) + 1) if M else 0,
        "hap": tags(terms, L, phase["hap"].tolist(), phase["set"].tolist(), n_events, int(max_sets)),
        "cis_ld": np.array(cld, dtype=np.longdouble).reshape(M, W), "trans_ld": np.array(tld, dtype=np.longdouble).reshape(M, W),
        "bound": bound(terms, L, W),
        "hap_ld": hld, "set_ld": sld, "nterm": nterm,
        "margin_zero": min(live) if live else np.inf,
        "margin_link": min(abs(v - float(min_link)) for v in live) if live else np.inf,
    }


def decided(want):
    """the precondition of (b): every vote with a term is more than MARGIN away from 0 and from min_link (long double scan)"""
    return want["margin_zero"] > MARGIN and want["margin_link"] > MARGIN


def worst(link, want):
    """the largest |cis or trans - long double| / bound over the pairs (0.0 without any): printed by the tests before they assert"""
    link = np.asarray(link)
    if not link.size:
        return 0.0
    err = np.maximum(np.abs(link["cis"].astype(np.longdouble) - want["cis_ld"]), np.abs(link["trans"].astype(np.longdouble) - want["trans_ld"])).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / want["bound"])
    return float(r.max())


def same_link(link, want):
    """the counts equal (reserved 0), cis and trans within the bound of the long double loop"""
    link, ref = np.asarray(link), want["link"]
    if link.dtype != _capi.EDIT_LINK or link.shape != ref.shape:
        return False
    if not all(np.array_equal(link[k], ref[k]) for k in ("n_both", "n_cis", "n_trans", "reserved")):
        return False
    ok = np.abs(link["cis"].astype(np.longdouble) - want["cis_ld"]) <= want["bound"]
    return bool(np.all(ok & (np.abs(link["trans"].astype(np.longdouble) - want["trans_ld"]) <= want["bound"])))


def same_phase(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and all(np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in got.dtype.names)


def check(got, want, scores, tag, exact=False):
    """every output of one ScoreMutationPhase result (scores, link, phase, hap, n_sets, scored list) against the yardstick; the
    figures are printed before anything is asserted.  exact: cis / trans byte for byte the float64 loop's (the fallback path)."""
    sc, link, phase, hap, n_sets, scored = got
    print("%s: worst |cis, trans - long double| / bound = %.4f; smallest |vote| %.3g, smallest ||vote| - min_link| %.3g" %
          (tag, worst(link, want), want["margin_zero"], want["margin_link"]))
    assert np.asarray(sc).dtype == np.float64 and np.asarray(sc).tobytes() == np.asarray(scores, dtype=np.float64).tobytes()
    assert S.score_bytes(scored) == np.asarray(sc).tobytes()
    assert same_link(link, want)
    if exact:
        assert same_phase(link, want["link"])
    assert same_phase(phase, replay(link, want["min_link"]) if want["M"] else want["phase"])          # (a)
    assert decided(want)                                                                              # (b): its precondition,
    assert phase["hap"].tolist() == want["hap_ld"] and phase["set"].tolist() == want["set_ld"]        #      then the decisions
    assert n_sets == want["n_sets"] == ((want["set_ld"][-1] + 1) if want["M"] else 0)
    assert phase["hap"].tolist() == want["phase"]["hap"].tolist() and phase["set"].tolist() == want["phase"]["set"].tolist()
    assert hap is not None and same_phase(hap, want["hap"])                                           # with the phase equal: by bytes


# ---- the cases, shared by the CPU and the GPU tests: test_phase.py asserts `decided` for every one of them, so that a seed that
# puts a vote near a threshold fails on the CPU before it is ever compared on the GPU
import copy

import backends as B
import tiled_cases as T
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS

P0 = dict(DEFAULT_PARAMS, verbose=0)
DIPLOID = {"400": (400, 10, 7701, (60, 150, 240, 330)), "260": (260, 8, 7702, (40, 47, 120, 200))}      # length, events, seed, sites
_MADE = {}


def region(L, E, seed):
    """(draft, events) of a synthetic region, made once"""
    if (L, E, seed) not in _MADE:
        _MADE[(L, E, seed)] = synth.make_region(L, E, seed, B.oracle_swalign, P0)[:2]
    return _MADE[(L, E, seed)]


def diploid(name):
    """synth.make_diploid_region of DIPLOID[name], made once: (draft, events, event haplotypes, edits, carriers)"""
    if ("diploid", name) not in _MADE:
        L, E, seed, sites = DIPLOID[name]
        _MADE[("diploid", name)] = synth.make_diploid_region(L, E, seed, B.oracle_swalign, sites, P0)
    return _MADE[("diploid", name)]


def shapes():
    """name -> (draft, events, params, sites, window, min_link, max_sets): the smallest shapes at which each kernel can go wrong"""
    d, e5 = region(120, 5, 7401)
    n = len(d)
    pts = S.point_list(d)
    inert = copy.deepcopy(e5)
    inert[2].ref_align[:] = 0                   # an event without alignment: no span, its Alignment is a no-op
    e257 = [copy.deepcopy(e5[i % 5]) for i in range(257)]      # the second SUP_EV staging pass of k_link
    gone = S.edit(n + 3, "A", "C")              # ScoreMutations skips it (start > L): nobody covers it
    dd, de, _eh, het, _car = diploid("400")
    dpts = S.point_list(dd)
    td, te, tp = T.crafted("single", "loader")
    mix = [het[(i // 3) % 4] if i % 3 == 0 else dpts[900 + 7 * i] for i in range(129)]      # (the library takes any list: het edits repeat)
    return {
        "M1": (d, e5, P0, pts[400:401], 2, 0.0, 4),
        "M2": (d, e5, P0, pts[400:402], 2, 0.0, 4),
        "M3_W2": (d, e5, P0, pts[410:413], 2, 0.0, 4),                      # M = W + 1
        "M9_W8": (d, e5, P0, pts[200:209], 8, 0.0, 4),
        "M255_W1": (d, e5, P0, pts[300:555], 1, 0.0, 4),
        "M256_W2": (d, e5, P0, pts[300:556], 2, 0.0, 4),
        "M257_W8": (d, e5, P0, pts[300:557], 8, 0.0, 8),                  # the partners of the first block's last sites lie in the next block's range
        "M0": (d, e5, P0, [], 2, 0.0, 4),
        "E1": (d, e5[:1], P0, pts[300:600], 2, 0.0, 4),
        "E257": (d, e257, P0, pts[230:300], 2, 0.0, 4),
        "inert_event": (d, inert, P0, pts[300:600], 2, 0.0, 4),
        # a site nobody covers opens a set without a term; the site behind it looks back across that break at a partner with shared events
        "skipped_site": (d, e5, P0, pts[300:306] + [gone] + pts[306:312], 4, 0.0, 4),
        "every_site_alone": (d, e5, P0, pts[500:512], 2, 1e300, 8),       # n_sets = M = 12 > max_sets
        # k_haptag: a list on the first diploid region with both haplotypes in every stretch of it, 63 .. 129 sites in one set (the
        # lanes' second and third terms), and cut by min_link into 14 sets, more than are tagged
        "M63_S1": (dd, de, P0, mix[:63], 2, 0.0, 1),
        "M64_S8": (dd, de, P0, mix[:64], 2, 0.0, 8),
        "M65_S1": (dd, de, P0, mix[:65], 3, 0.0, 1),
        "M129_S8": (dd, de, P0, mix, 2, 0.0, 8),
        "sets14_S8": (dd, de, P0, mix, 2, 5.0, 8),
        "sets14_S1": (dd, de, P0, mix, 2, 5.0, 1),
        "no_events": (d, [], P0, pts[300:310], 2, 0.0, 4),               # written on the host: the rules on all-zero links
        # partial-span reads (tiled_cases "single"): pairs shared by one to four of the five events.  (Its interior: at the region's
        # ends the one covering read's terms are exactly 0.0 and so are the votes, which (b)'s precondition does not admit.)
        "tiled_single": (td, te, tp, sorted([m for m in T.edits(td, te, 5) if 100 <= m.start <= 330], key=lambda m: m.start), 4, 0.0, 4),
    }


def want_of(key, draft, events, par, sites, window, min_link, max_sets):
    """(the yardstick, support_cases' scores) of one case, computed once"""
    def make():
        terms = S.oracle_terms(draft, events, par, sites)
        scores = np.zeros(len(sites))
        for m in range(len(sites)):
            s = -1e-6
            for e in range(len(events)):
                s += terms[1][e][m]
            scores[m] = s
        return yardstick(terms, len(draft), len(events), window, min_link, max_sets), scores
    return T.oracle_once(("phase",) + tuple(key), make)


# the three regions of test_batch._split_case (the middle one without events) for the split paths of the chain: per region the
# window, min_link and max_sets
SPLIT_KW = dict(window=[3, 2, 1], min_link=[0.0, 0.0, 2.0], max_sets=[2, 4, 8])


def split_wants():
    """[(key, yardstick, scores)] of both phase calls of the split test: on _split_case's support lists (one empty) and on its
    ScoreMutations lists (none empty), three regions each"""
    from test_batch import _split_case, P
    regs, sup_lists, sm_lists, _groups = _split_case()
    out = []
    for k, lists in enumerate((sup_lists, sm_lists)):
        for i, ((d, ev), sites) in enumerate(zip(regs, lists)):
            out.append(((k, i),) + want_of(("split", k, i), d, ev, P, sites, SPLIT_KW["window"][i], SPLIT_KW["min_link"][i], SPLIT_KW["max_sets"][i]))
    return out


# ---- consensus.variant_support(phase=True) on the two diploid regions: the call both test files make, and the records it has to write
VARIANT_STARTS = (1000, 5000)


def variant_lists():
    """per diploid region the candidate list with absolute starts: its four het edits in order with two edits that no read carries
    (a substitution at 20, an insertion at 100) among them"""
    out = []
    for name, s0 in zip(("400", "260"), VARIANT_STARTS):
        dr, _ev, _eh, edits, _car = diploid(name)
        extra = [S.edit(20, dr[20], "A" if dr[20] != "A" else "C"), S.edit(100, "", "G")]
        out.append([S.edit(s0 + m.start, m.orig, m.mut) for m in (extra[:1] + edits[:2] + extra[1:] + edits[2:])])
    return out


VARIANT_KW = dict(region_starts=list(VARIANT_STARTS), fmt="vcf", chrom=["ctgA", "ctgB"], ploidy=2, sample="s1", min_score=-1e9)
VARIANT_PS_LINE = ('##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set: POS of the first site of the set of phased het sites the record '
                   'belongs to (uncalibrated)">')
VARIANT_BODY = (
    'ctgA\t1021\t.\tG\tA\t0\t.\tLLR=-176.91140948801558;DP=10;GDP=5,5;GSUP=0,0;GOPP=5,5;GLLR=-90.96510310179349,-85.9463053862221\tGT:GQ:PL:PS\t0/0:30:0,30,768:.\n'
    'ctgA\t1061\t.\tT\tC\t76\t.\tLLR=17.551710397500415;DP=10;GDP=5,5;GSUP=0,5;GOPP=5,0;GLLR=-91.44714591245497,108.99885730995538\tGT:GQ:PL:PS\t1|0:99:443,0,367:1061\n'
    'ctgA\t1151\t.\tG\tT\t0\t.\tLLR=-2.2364056337897864;DP=10;GDP=5,5;GSUP=5,0;GOPP=0,5;GLLR=128.22587942116104,-130.46228405495083\tGT:GQ:PL:PS\t0|1:99:527,0,536:1061\n'
    'ctgA\t1100\t.\tT\tTG\t0\t.\tLLR=-177.71491419241408;DP=10;GDP=5,5;GSUP=0,0;GOPP=5,5;GLLR=-85.56490513863832,-92.15000805377576\tGT:GQ:PL:PS\t0/0:30:0,30,772:.\n'
    'ctgA\t1241\t.\tG\tC\t0\t.\tLLR=-18.028191712768717;DP=10;GDP=5,5;GSUP=0,5;GOPP=5,0;GLLR=-125.457296362433,107.42910564966428\tGT:GQ:PL:PS\t1|0:99:436,0,515:1061\n'
    'ctgA\t1331\t.\tT\tA\t87\t.\tLLR=20.086772460502402;DP=10;GDP=5,5;GSUP=5,0;GOPP=0,5;GLLR=107.74868532579353,-87.66191186529113\tGT:GQ:PL:PS\t0|1:99:438,0,351:1061\n'
    'ctgB\t5021\t.\tC\tA\t0\t.\tLLR=-89.54910095468551;DP=8;GDP=4,4;GSUP=0,0;GOPP=4,4;GLLR=-45.06458711160781,-44.48451284307771\tGT:GQ:PL:PS\t0/0:23:0,23,389:.\n'
    'ctgB\t5041\t.\tC\tT\t0\t.\tLLR=-19.070713958294732;DP=8;GDP=4,4;GSUP=0,4;GOPP=4,0;GLLR=-91.65532140420885,72.58460844591411\tGT:GQ:PL:PS\t1|0:99:291,0,374:5041\n'
    'ctgB\t5048\t.\tA\tG\t0\t.\tLLR=-9.18805861204601;DP=8;GDP=4,4;GSUP=4,0;GOPP=0,4;GLLR=84.98890395641615,-94.17696156846216\tGT:GQ:PL:PS\t0|1:99:345,0,385:5041\n'
    'ctgB\t5100\t.\tA\tAG\t0\t.\tLLR=-163.86886347265624;DP=8;GDP=4,4;GSUP=0,0;GOPP=4,4;GLLR=-76.68464688078018,-87.18421559187607\tGT:GQ:PL:PS\t0/0:24:0,24,712:.\n'
    'ctgB\t5121\t.\tG\tA\t0\t.\tLLR=-8.016661492059772;DP=8;GDP=4,4;GSUP=0,4;GOPP=4,0;GLLR=-80.75926791971557,72.7426074276558\tGT:GQ:PL:PS\t1|0:99:292,0,327:5041\n'
    'ctgB\t5201\t.\tC\tG\t103\t.\tLLR=23.613894664821316;DP=8;GDP=4,4;GSUP=4,0;GOPP=0,4;GLLR=97.70817841615008,-74.09428275132876\tGT:GQ:PL:PS\t0|1:99:400,0,298:5041\n')
