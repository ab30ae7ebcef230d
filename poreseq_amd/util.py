"""Boundary value types with the reference's shapes (poreseq/Util.py:2-111, Params.py:4-29).

`poreseqcpp.PSAlign` hands these out and accepts them exactly as the reference's
Cython module does (`from Util import MutationInfo, MutationScore`, pyx:13).
"""


class RegionInfo:
    """'name', 'start:end' or 'name:start:end' (poreseq/Util.py:2-33)."""

    def __init__(self, region=None):
        self.start = None
        self.end = None
        self.name = None
        if region is None:
            return
        parts = region.split(':')
        if len(parts) != 2:
            self.name = parts[0]
        if len(parts) > 1:
            self.start = int(parts[-2])
            self.end = int(parts[-1])


def _dot(s):
    return s if len(s) else '.'


class MutationInfo:
    """0-based start, original bases, mutated bases ('' for none) (poreseq/Util.py:35-81)."""

    def __init__(self, info=None):
        self.start = 0
        self.orig = ""
        self.mut = ""
        if info is None:
            return
        if len(info) == 0 or info[0] == '#':
            self.start = -1
            return
        vals = info.split()
        if len(vals) != 3:
            self.start = -1
            return
        self.start = int(vals[0])
        self.orig = '' if vals[1] == '.' else vals[1]
        self.mut = '' if vals[2] == '.' else vals[2]

    def __str__(self):
        return '{}\t{}\t{}'.format(self.start, _dot(self.orig), _dot(self.mut))


class MutationScore:
    """A MutationInfo plus the summed log-likelihood change (poreseq/Util.py:83-111)."""

    def __init__(self):
        self.start = 0
        self.orig = ""
        self.mut = ""
        self.score = 0

    def __str__(self):
        return '{}\t{}\t{}\t{}'.format(self.start, _dot(self.orig), _dot(self.mut), self.score)


# defaults.conf:1-19 of the reference
DEFAULT_PARAMS = {
    'realign_width': 300.0, 'scoring_width': 100.0, 'point_width': 20.0,
    'min_coverage': 0.0, 'max_coverage': 30.0, 'min_overlap': 500.0, 'max_length': 10000.0,
    'end_trim': 150.0, 'lik_offset': 4.5,
    'skip_t': 0.141, 'skip_c': 0.088, 'stay_t': 0.043, 'stay_c': 0.057,
    'extend_t': 0.072, 'extend_c': 0.046, 'insert_t': 0.020, 'insert_c': 0.025,
}


def LoadParams(filename):
    """`key = float` lines; anything else is skipped silently (poreseq/Params.py:4-23)."""
    params = {}
    if filename is None:
        return params
    with open(filename) as f:
        for line in f:
            kv = line.split('=')
            if len(kv) == 2:
                try:
                    params[kv[0].strip()] = float(kv[1])
                except ValueError:
                    pass
    return params


def VaryParams(params, n=16, picks=3, spread=0.15):
    """One training iteration's candidate parameter sets (poreseq/Params.py:31-60): `n` copies of `params`, each with
    `picks` distinct transition parameters (keys ending in _t / _c, in dict order) multiplied by a Gaussian factor
    N(1, spread).  Draws come from Python's global `random`, one `sample` then `picks` `gauss` calls per copy — the
    reference's order, so a seeded generator gives the reference's list."""
    import random
    tunable = [k for k in params.keys() if k.endswith('_t') or k.endswith('_c')]
    out = []
    for _ in range(n):
        cand = params.copy()
        for k in random.sample(tunable, picks):
            cand[k] *= random.gauss(1.0, spread)
        out.append(cand)
    return out


def SaveParams(filename, params):
    with open(filename, 'w') as f:
        for p in params:
            f.write('{} = {}\n'.format(p, params[p]))


def phred_from_margin(margin, length):
    """Per-base qualities uint8 [length] of a consensus from PointTable's `margin` (the largest point-edit score per position):
    Q = clip(floor(-margin * 10 / ln 10 + 0.5), 0, 93).  The scores are natural-log likelihood ratios, so this is the Phred scale
    of the ratio between the called base and its best single-base alternative (deletion, substitution or insertion in front of
    it); 93 is the top of FASTQ's printable range.  Positions without a row — the last four bases, which FindPointMutations does
    not walk — get 0, and so does a position whose best alternative scores >= 0.
    UNCALIBRATED: a likelihood ratio of this model, not a measured error rate; it orders bases by confidence and no more."""
    import numpy as np
    m = np.asarray(margin, dtype=np.float64)
    q = np.zeros(int(length), dtype=np.uint8)
    k = min(m.size, int(length))
    with np.errstate(invalid='ignore', over='ignore'):
        v = np.clip(np.floor(-m[:k] * 10.0 / np.log(10.0) + 0.5), 0, 93)
    q[:k] = np.where(np.isnan(v), 0, v).astype(np.uint8)
    return q


def write_fastq(out, name, seq, qual):
    """One FASTQ record: '@name', the sequence, '+', chr(33 + q) per base."""
    if len(qual) != len(seq):
        raise ValueError("write_fastq: %d qualities for %d bases" % (len(qual), len(seq)))
    out.write('@{}\n{}\n+\n{}\n'.format(name, seq, ''.join(chr(33 + int(q)) for q in qual)))


def support_groups(events, groups=None, n_groups=None):
    """(group ids int32 [E], G) of a support call (PSAlign.ScoreMutationSupport): `groups` defaults to the strand of every event
    (0 template, 1 complement, from ev.model.complement) and `n_groups` to 2 for that default, otherwise to the largest id + 1.
    ValueError for a list that is not one id per event, G outside 1 .. 8 or an id outside 0 .. G - 1."""
    import numpy as np
    E = len(events)
    if groups is None:
        groups = [1 if getattr(ev.model, 'complement', False) else 0 for ev in events]
        if n_groups is None:
            n_groups = 2
    grp = np.asarray(list(groups), dtype=np.int64).reshape(-1)
    if grp.size != E:
        raise ValueError("support: %d group ids for %d events" % (grp.size, E))
    G = int(n_groups) if n_groups is not None else (int(grp.max()) + 1 if E else 1)
    if not 1 <= G <= 8:
        raise ValueError("support: n_groups = %d, allowed are 1 .. 8" % G)
    bad = np.flatnonzero((grp < 0) | (grp >= G))
    if bad.size:
        raise ValueError("support: event %d has group %d, n_groups = %d" % (int(bad[0]), int(grp[bad[0]]), G))
    return grp.astype(np.int32), G


def spans_from_refs(ref_aligns):
    """int64 [E, 2]: (refstart, refend) of every event — the int of the first and of the last positive entry of its ref_align
    (cpp/EventData.h:110-169) — and (1, 0), an empty span, for an event without a positive entry."""
    import numpy as np
    out = np.empty((len(ref_aligns), 2), dtype=np.int64)
    for e, ra in enumerate(ref_aligns):
        on = np.asarray(ra)[np.asarray(ra) > 0]
        out[e] = (int(on[0]), int(on[-1])) if on.size else (1, 0)
    return out


def support_from_deltas(deltas, groups, n_groups, spans, starts, seq_len):
    """The definition of what ps_score_mutation_support returns, in numpy — and the path of a library without the entry point.
    deltas [E, M]: every event's term of every edit's score (ScoreMutationDeltas); groups [E] ids in 0 .. n_groups - 1;
    spans [E, 2]: (refstart, refend) of the events as re-aligned by that call, empty (refstart > refend) for an event without
    alignment (`spans_from_refs`); starts [M] the edits' starts; seq_len the length of the sequence they edit.
    Returns (scores float64 [M], support [M, n_groups] of _capi.EDIT_SUPPORT):
      scores   -1e-6 plus all events' terms in event order (the bits of ScoreMutations)
      sum      0.0 plus the terms of the group's events in event order, covering or not
      cover    events of the group with refstart <= start + 1 <= refend; an edit with start > seq_len (skipped by ScoreMutations) has none
      pos/neg  those of them with a term > 0 / < 0
    `cover` is a span test, not a likelihood test: a covering read's term can be zero and a read's term is not zero outside its span."""
    import numpy as np
    from ._capi import EDIT_SUPPORT
    deltas = np.asarray(deltas, dtype=np.float64)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    E, M = (deltas.shape[0], starts.size) if deltas.ndim == 2 else (0, starts.size)
    deltas = deltas.reshape(E, M)
    grp = np.asarray(groups, dtype=np.int64).reshape(-1)
    G = int(n_groups)
    if grp.size != E or not 1 <= G <= 8 or np.any((grp < 0) | (grp >= G)):
        raise ValueError("support_from_deltas: groups / n_groups")
    spans = np.asarray(spans, dtype=np.int64).reshape(E, 2)
    col = starts + 1
    live = starts <= int(seq_len)
    scores = np.full(M, -1e-6, dtype=np.float64)
    sup = np.zeros((M, G), dtype=EDIT_SUPPORT)
    for e in range(E):
        d = deltas[e]
        scores = scores + d
        g = int(grp[e])
        sup['sum'][:, g] = sup['sum'][:, g] + d
        cv = live & (spans[e, 0] <= col) & (col <= spans[e, 1])
        sup['cover'][:, g] += cv
        sup['pos'][:, g] += cv & (d > 0)
        sup['neg'][:, g] += cv & (d < 0)
    return scores, sup


def alt_fractions(ploidy):
    """The alt-allele fractions of the heterozygous genotypes of a sample with `ploidy` copies: [k / ploidy for k in 1 .. ploidy - 1]
    (empty for ploidy 1: hom-ref and hom-alt need none).  ValueError outside 1 .. 9 — a genotype call takes at most 8 fractions."""
    P = int(ploidy)
    if P != ploidy or not 1 <= P <= 9:
        raise ValueError("alt_fractions: ploidy = %r, allowed are 1 .. 9" % (ploidy,))
    return [k / P for k in range(1, P)]


def check_alt_frac(alt_frac):
    """float64 [K] of the alt fractions of a genotype call; ValueError for more than 8 or one outside 1e-6 .. 1 - 1e-6 (NaN included)"""
    import numpy as np
    f = np.asarray(list(alt_frac), dtype=np.float64).reshape(-1)
    if f.size > 8:
        raise ValueError("genotypes: n_frac = %d, allowed are 0 .. 8" % f.size)
    bad = np.flatnonzero(~((f >= 1e-6) & (f <= 1.0 - 1e-6)))
    if bad.size:
        raise ValueError("genotypes: alt_frac[%d] = %g, allowed is 1e-06 .. 1 - 1e-06" % (int(bad[0]), float(f[bad[0]])))
    return f


def genotypes_from_deltas(deltas, spans, starts, seq_len, alt_frac):
    """The definition of what ps_score_mutation_genotypes adds to the support call, in numpy float64 — and the path of a library
    without the entry point.  deltas [E, M], spans [E, 2], starts [M], seq_len as `support_from_deltas` takes them; alt_frac the K
    alt-allele fractions f_k (0 .. 8 of them, each 1e-6 .. 1 - 1e-6), g_k = 1.0 - f_k.
    Returns (lik float64 [M, K + 1], n_cover int32 [M]).  Only the events that COVER an edit (support_from_deltas' test) enter:
      n_cover     the number of covering events
      lik[:, k]   0.0, then for e ascending with cover:  d = delta[e][m], u = exp(-|d|), x = g_k u + f_k if d > 0 else g_k + f_k u,
                  += (d if d > 0 else 0.0) + log(x) — log((1 - f) + f e^d) without a positive exponent.  d = -inf adds log(g_k),
                  d = +inf gives +inf, NaN gives NaN.
      lik[:, K]   0.0, then += d over the covering events in event order: hom-alt, every covering read carries the edit.
    Hom-ref is 0 by construction.  An edit with start > seq_len and every edit without covering events has n_cover 0 and lik 0."""
    import numpy as np
    deltas = np.asarray(deltas, dtype=np.float64)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    E, M = (deltas.shape[0], starts.size) if deltas.ndim == 2 else (0, starts.size)
    deltas = deltas.reshape(E, M)
    f = check_alt_frac(alt_frac)
    g = 1.0 - f
    K = f.size
    spans = np.asarray(spans, dtype=np.int64).reshape(E, 2)
    col = starts + 1
    live = starts <= int(seq_len)
    lik = np.zeros((M, K + 1), dtype=np.float64)
    n_cover = np.zeros(M, dtype=np.int32)
    with np.errstate(all='ignore'):
        for e in range(E):
            cv = live & (spans[e, 0] <= col) & (col <= spans[e, 1])
            if not cv.any():
                continue
            d = deltas[e][cv]
            up = d > 0
            u = np.exp(-np.abs(d))
            top = np.where(up, d, 0.0)
            for k in range(K):
                x = np.where(up, g[k] * u + f[k], g[k] + f[k] * u)
                lik[cv, k] = lik[cv, k] + (top + np.log(x))
            lik[cv, K] = lik[cv, K] + d
            n_cover[cv] += 1
    return lik, n_cover


def call_genotypes(lik, n_cover, ploidy):
    """(GT strings [M], GQ ints [M], PL lists [M][ploidy + 1]) from the likelihoods of a genotype call made with
    alt_fractions(ploidy).  Host only.  Genotype k is the number of alt copies, 0 .. P: L_0 = 0 (hom-ref), L_k = lik[:, k - 1],
    L_P = lik[:, -1] (hom-alt).  PL_k = min(int(floor(-10 (L_k - max L) / ln 10 + 0.5)), 9999); GT is the first k that holds the
    maximum, written as (P - k) zeros then k ones joined by '/' ('0/0', '0/1', '1/1' for P = 2; '0' or '1' for P = 1);
    GQ = min(99, second smallest PL).  An edit with n_cover == 0 or a NaN among its L is a no-call: '.' repeated P times, GQ 0,
    all PL 0.  UNCALIBRATED, like QUAL and the FASTQ qualities: ratios of this model's likelihoods, not measured error rates."""
    import math
    import numpy as np
    P = len(alt_fractions(ploidy)) + 1
    lik = np.asarray(lik, dtype=np.float64)
    n_cover = np.asarray(n_cover).reshape(-1)
    if lik.size != n_cover.size * P or (lik.ndim == 2 and lik.shape[1] != P):     # (an empty list has no rows to call: three empty lists)
        raise ValueError("call_genotypes: ploidy %d needs %d likelihood columns per edit" % (P, P))
    gts, gqs, pls = [], [], []
    for row, nc in zip(lik.reshape(n_cover.size, P).tolist(), n_cover.tolist()):
        L = [0.0] + row
        if nc == 0 or any(v != v for v in L):
            gts.append('/'.join(['.'] * P))
            gqs.append(0)
            pls.append([0] * (P + 1))
            continue
        top = max(L)
        k = L.index(top)
        pl = []
        for v in L:
            q = 0.0 if v == top else -10.0 * (v - top) / math.log(10.0)     # (an infinite maximum: 0 for itself, the cap for the rest)
            pl.append(9999 if not q < 9999.0 else min(int(math.floor(q + 0.5)), 9999))
        gts.append('/'.join(['0'] * (P - k) + ['1'] * k))
        gqs.append(min(99, sorted(pl)[1]))
        pls.append(pl)
    return gts, gqs, pls


def check_phase_args(window, min_link, max_sets):
    """(W, min_link, S) of a phase call; ValueError for a window outside 1 .. 8, max_sets outside 1 .. 8 or a min_link that is negative
    or not finite (NaN included)"""
    W, S, v = int(window), int(max_sets), float(min_link)
    if W != window or not 1 <= W <= 8:
        raise ValueError("phase: window = %r, allowed are 1 .. 8" % (window,))
    if S != max_sets or not 1 <= S <= 8:
        raise ValueError("phase: max_sets = %r, allowed are 1 .. 8" % (max_sets,))
    if not (v >= 0.0 and v <= 1.7976931348623157e308):
        raise ValueError("phase: min_link = %r, allowed is a finite value >= 0" % (min_link,))
    return W, v, S


def phase_scan(link, min_link):
    """The phase scan of ps_score_mutation_phase on link records [M, W] (_capi.EDIT_LINK), in float64 — the rule is defined on the
    records alone, so this replays a device result bit for bit.  Site 0: vote 0.0, hap +1, set 0.  Site m > 0: vote = 0.0; for
    w = 1 .. min(W, m) with i = m - w and L = link[i, w - 1]: if set[i] == set[m - 1] and L.n_both > 0, vote += hap[i] * (L.cis -
    L.trans).  vote != 0 and |vote| >= min_link (a NaN fails both): the site joins set[m - 1] with hap = +1 if vote > 0 else -1;
    otherwise it opens set[m - 1] + 1 with hap +1.  Returns (phase [M] of _capi.EDIT_PHASE, n_sets)."""
    import numpy as np
    from ._capi import EDIT_PHASE
    link = np.asarray(link)
    M = link.shape[0]
    W = link.shape[1] if link.ndim == 2 else 0
    phase = np.zeros(M, dtype=EDIT_PHASE)
    if not M:
        return phase, 0
    cis, trans, both = link["cis"].tolist(), link["trans"].tolist(), link["n_both"].tolist()
    hap, sets, votes = [1], [0], [0.0]
    lim = float(min_link)
    for m in range(1, M):
        vote = 0.0
        for w in range(1, min(W, m) + 1):
            i = m - w
            if sets[i] == sets[m - 1] and both[i][w - 1] > 0:
                vote = vote + hap[i] * (cis[i][w - 1] - trans[i][w - 1])
        if vote != 0.0 and abs(vote) >= lim:
            sets.append(sets[m - 1])
            hap.append(1 if vote > 0 else -1)
        else:
            sets.append(sets[m - 1] + 1)
            hap.append(1)
        votes.append(vote)
    phase["vote"], phase["hap"], phase["set"] = votes, hap, sets
    return phase, sets[-1] + 1


def phase_from_deltas(deltas, spans, starts, seq_len, window, min_link, max_sets):
    """The definition of what ps_score_mutation_phase reduces on the device, in numpy float64 — and the path of a library without the
    entry point.  deltas [E, M], spans [E, 2], starts [M], seq_len as `support_from_deltas` takes them (cover is its test); window W
    in 1 .. 8, min_link finite and >= 0, max_sets S in 1 .. 8.
    Returns (link [M, W] of _capi.EDIT_LINK, phase [M] of _capi.EDIT_PHASE, hap [E, S] of _capi.EVENT_HAP, n_sets):
      link[m, w - 1]  the pair (m, j = m + w), all zero where j >= M.  Over the events e ascending that cover both, da = delta[e][m],
                      db = delta[e][j], s = da + db, r = da - db:  cis += (s if s > 0 else 0.0) + log(0.5 + 0.5 exp(-|s|)) — both
                      alts on one copy —, trans += max(da, db) + log(0.5 + 0.5 exp(-|r|)) — one on each —, n_both counts the events,
                      n_cis those with both terms > 0 or both < 0, n_trans those with one > 0 and the other < 0.
      phase           `phase_scan` of the links.
      hap[e, k]       over the sites m of set k (k < S) that e covers: lik1 / n1 sum and count those with hap +1, lik2 / n2 those
                      with hap -1; the adds run as the device runs them — partial l = 0.0 plus the terms of m = l, l + 64, ...
                      ascending, then the 64 partials into 0.0 in order.
    The model treats an edit's terms as independent of the other edit of a pair; everything derived is uncalibrated."""
    import numpy as np
    from ._capi import EDIT_LINK, EVENT_HAP
    W, lim, S = check_phase_args(window, min_link, max_sets)
    deltas = np.asarray(deltas, dtype=np.float64)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    E, M = (deltas.shape[0], starts.size) if deltas.ndim == 2 else (0, starts.size)
    deltas = deltas.reshape(E, M)
    spans = np.asarray(spans, dtype=np.int64).reshape(E, 2)
    col = starts + 1
    live = starts <= int(seq_len)
    cover = live[None, :] & (spans[:, :1] <= col[None, :]) & (col[None, :] <= spans[:, 1:])      # [E, M]
    link = np.zeros((M, W), dtype=EDIT_LINK)
    with np.errstate(all='ignore'):
        for w in range(1, W + 1):
            n = M - w
            if n <= 0:
                break
            cis, trans = np.zeros(n), np.zeros(n)
            for e in range(E):
                both = cover[e, :n] & cover[e, w:]
                if not both.any():
                    continue
                da, db = deltas[e, :n][both], deltas[e, w:][both]
                s, r = da + db, da - db
                cis[both] = cis[both] + (np.where(s > 0, s, 0.0) + np.log(0.5 + 0.5 * np.exp(-np.abs(s))))
                trans[both] = trans[both] + (np.where(da > db, da, db) + np.log(0.5 + 0.5 * np.exp(-np.abs(r))))
                link["n_both"][:n, w - 1][both] += 1
                link["n_cis"][:n, w - 1][both] += ((da > 0) & (db > 0)) | ((da < 0) & (db < 0))
                link["n_trans"][:n, w - 1][both] += ((da > 0) & (db < 0)) | ((da < 0) & (db > 0))
            link["cis"][:n, w - 1], link["trans"][:n, w - 1] = cis, trans
    phase, n_sets = phase_scan(link, lim)
    hap = np.zeros((E, S), dtype=EVENT_HAP)
    rows = (M + 63) // 64
    pad = rows * 64 - M
    d = np.pad(deltas, ((0, 0), (0, pad))).reshape(E, rows, 64)
    for k in range(min(S, n_sets)):
        for sign, lik, cnt in ((1, "lik1", "n1"), (-1, "lik2", "n2")):
            member = cover & ((phase["set"] == k) & (phase["hap"] == sign))[None, :]
            mk = np.pad(member, ((0, 0), (0, pad))).reshape(E, rows, 64)
            part = np.zeros((E, 64))
            for row in range(rows):
                part = part + np.where(mk[:, row], d[:, row], 0.0)      # (+0.0 leaves a sum that began at +0.0 as it is)
            tot = np.zeros(E)
            for lane in range(64):
                tot = tot + part[:, lane]
            hap[lik][:, k] = tot
            hap[cnt][:, k] = member.sum(axis=1)
    return link, phase, hap, n_sets


def call_phase(gts, phase, pos=None):
    """(phased GT strings [M], PS values [M]) from the unphased genotypes of the sites of one phase call and its phase records
    (_capi.EDIT_PHASE).  A '0/1' site in a phase set of two or more sites becomes '1|0' (hap +1: its alt is on the copy that
    carries the alt of the set's first site) or '0|1' (hap -1), and its PS is that of the set: pos[first site of the set] — the VCF
    POS when `pos` holds the sites' POS — or, without `pos`, the first site's index.  A site alone in its set, and every GT that is
    not '0/1', stays as it is with PS None.  Host only; uncalibrated, like the votes it rests on."""
    import numpy as np
    gts = list(gts)
    phase = np.asarray(phase)
    if phase.shape != (len(gts),):
        raise ValueError("call_phase: %d genotypes for %d phase records" % (len(gts), phase.size))
    sets, haps = phase["set"].tolist(), phase["hap"].tolist()
    first, size = {}, {}
    for m, k in enumerate(sets):
        first.setdefault(k, m)
        size[k] = size.get(k, 0) + 1
    out, ps = [], []
    for m, (gt, k, h) in enumerate(zip(gts, sets, haps)):
        if gt != '0/1' or size[k] < 2:
            out.append(gt)
            ps.append(None)
            continue
        out.append('1|0' if h > 0 else '0|1')
        ps.append(first[k] if pos is None else pos[first[k]])
    return out, ps


def align_stats_from_refs(states, mean, ra, level_mean, level_stdv):
    """One event's ps_event_stats record (_capi.EVENT_STATS, shape ()) — the definition of include/poreseq_hip.h in numpy float64, and
    the path of a library without ps_align_stats.  states: the 5-mer states of the sequence (states[j - 1] belongs to column j);
    mean, ra: the event's level means and ref_align; level_mean, level_stdv: its model rows.
    A level is aligned iff ra > 0, inserted iff ra < 0, unaligned otherwise; its column is c = int(min(ra, 2147483647.0)).  The
    census compares every aligned level's column with that of the aligned level before it (d = 0: stay, or extend when that one
    was itself a repeat; 1: step; > 1: jump over d - 1 columns; < 0: back); it is a census of the array, not of the path's moves.
    An aligned level with 1 <= c <= len(states) and states[c - 1] >= 0 enters the fit with w = 1 / s_k^2, wm = w m_k, r = mean - m_k:
    sw, swm, swmm, swr, swmr, swrr are the sums of w, wm, wm m_k, w r, wm r, (w r) r, added as the device adds them — partial t =
    0.0 plus the terms of the levels t, t + 256, ... ascending, then the 256 partials into 0.0 in order."""
    import numpy as np
    from ._capi import EVENT_STATS
    states = np.asarray(states, dtype=np.int64).reshape(-1)
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    ra = np.asarray(ra, dtype=np.float64).reshape(-1)
    lm = np.asarray(level_mean, dtype=np.float64).reshape(-1)
    ls = np.asarray(level_stdv, dtype=np.float64).reshape(-1)
    n, S = ra.size, states.size
    rec = np.zeros((), dtype=EVENT_STATS)
    with np.errstate(all='ignore'):
        al = ra > 0
        rec["n_levels"], rec["n_aligned"], rec["n_insert"] = n, int(al.sum()), int((ra < 0).sum())
        rec["n_unaligned"] = n - int(rec["n_aligned"]) - int(rec["n_insert"])
        col = np.zeros(n, dtype=np.int64)
        col[al] = np.minimum(ra[al], 2147483647.0).astype(np.int64)
        c = col[al]
        if c.size:
            rec["first_col"], rec["last_col"] = c[0], c[-1]
            d = np.diff(c)
            rep = d == 0
            prev_rep = np.concatenate([[False], rep[:-1]])
            rec["n_extend"], rec["n_stay"] = int((rep & prev_rep).sum()), int((rep & ~prev_rep).sum())
            rec["n_step"], rec["n_jump"], rec["n_back"] = int((d == 1).sum()), int((d > 1).sum()), int((d < 0).sum())
            rec["n_gap_cols"] = int((d[d > 1] - 1).sum())
        k = np.full(n, -1, dtype=np.int64)
        has = al & (col >= 1) & (col <= S)
        k[has] = states[col[has] - 1]
        fit = has & (k >= 0) & (k < lm.size)
        rec["n_fit"] = int(fit.sum())
        rec["n_nostate"] = int(rec["n_aligned"]) - int(rec["n_fit"])
        kk = np.where(fit, k, 0)
        mk, sk = lm[kk], ls[kk]
        w = 1.0 / (sk * sk)
        wm = w * mk
        r = mean - mk
        rows = (n + 255) // 256
        pad = rows * 256 - n
        tile = lambda a: np.pad(np.where(fit, a, 0.0), (0, pad)).reshape(rows, 256)
        for name, term in (("sw", w), ("swm", wm), ("swmm", wm * mk), ("swr", w * r), ("swmr", wm * r), ("swrr", (w * r) * r)):
            t = tile(term)
            part = np.zeros(256)
            for row in range(rows):
                part = part + t[row]      # (+0.0 for a level that does not enter leaves a sum that began at +0.0 as it is)
            tot = np.float64(0.0)
            for lane in range(256):
                tot = tot + part[lane]
            rec[name] = tot
    return rec


class ScalingFit(tuple):
    """(scale, shift, var, ok, n_fit) of fit_scaling, with the fields by name"""
    __slots__ = ()
    _fields = ("scale", "shift", "var", "ok", "n_fit")

    def __new__(cls, scale, shift, var, ok, n_fit):
        return tuple.__new__(cls, (float(scale), float(shift), float(var), bool(ok), int(n_fit)))

    scale = property(lambda self: self[0])
    shift = property(lambda self: self[1])
    var = property(lambda self: self[2])
    ok = property(lambda self: self[3])
    n_fit = property(lambda self: self[4])

    def __repr__(self):
        return "ScalingFit(scale=%r, shift=%r, var=%r, ok=%r, n_fit=%r)" % tuple(self)


def fit_scaling(stats, min_levels=100, min_spread=1e-6, scale_limits=(0.5, 2.0), var_limits=(0.25, 4.0)):
    """The shift / scale / var refit of one read's model from its ps_event_stats record (or a list of fits for an array of
    records): the weighted least-squares line of the residuals r = mean - m_k against the model means m_k, weights 1 / s_k^2:
        det = sw swmm - swm^2;  da = (sw swmr - swm swr) / det;  db = (swmm swr - swm swmr) / det;
        scale = 1 + da;  shift = db;  rss = swrr - da swmr - db swr;  var = sqrt(max(rss, 0) / n_fit)
    so that level_mean * scale + shift fits the read's levels, and level_stdv * var their scatter.  Returns ScalingFit(scale, shift,
    var, ok, n_fit).  ok iff n_fit >= min_levels, det > min_spread * sw * swmm (the aligned states' means are spread out enough to
    tell a scale from a shift) and scale / var lie inside their limits (and are finite); a fit that is not ok is the identity
    (1, 0, 1).  The limits are guards with documented defaults — a read whose refit leaves them is more likely misaligned than
    mis-scaled — not measurements.  Host only; drift and transition parameters are not fitted; the stdv channel's scale_sd / var_sd and
    per-k-mer re-estimation are fit_scaling_sd's and fit_kmers', from ps_kmer_stats' tables."""
    import math
    import numpy as np
    if isinstance(stats, np.ndarray) and stats.ndim > 0:
        return [fit_scaling(s, min_levels, min_spread, scale_limits, var_limits) for s in stats.reshape(-1)]
    n_fit = int(stats["n_fit"])
    sw, swm, swmm, swr, swmr, swrr = (float(stats[k]) for k in ("sw", "swm", "swmm", "swr", "swmr", "swrr"))
    ident = ScalingFit(1.0, 0.0, 1.0, False, n_fit)
    det = sw * swmm - swm * swm
    if n_fit < int(min_levels) or n_fit <= 0 or not (det > float(min_spread) * sw * swmm) or not math.isfinite(det):
        return ident
    da = (sw * swmr - swm * swr) / det
    db = (swmm * swr - swm * swmr) / det
    scale, shift = 1.0 + da, db
    rss = swrr - da * swmr - db * swr
    var = math.sqrt(max(rss, 0.0) / n_fit) if rss == rss else float("nan")
    if not (math.isfinite(scale) and math.isfinite(shift) and math.isfinite(var)):
        return ident
    if not (scale_limits[0] <= scale <= scale_limits[1] and var_limits[0] <= var <= var_limits[1]):
        return ident
    return ScalingFit(scale, shift, var, True, n_fit)


def apply_scaling(event, fit, var=True):
    """Apply a ScalingFit to an event's model in place: level_mean = level_mean * scale + shift and, with var, level_stdv =
    level_stdv * var.  Nothing else of the event or the model is touched (new arrays: a table shared with another model object
    is not written through)."""
    import numpy as np
    m = event.model
    m.level_mean = np.asarray(m.level_mean, dtype=np.float64) * float(fit.scale) + float(fit.shift)
    if var:
        m.level_stdv = np.asarray(m.level_stdv, dtype=np.float64) * float(fit.var)
    return event


# ---- per-k-mer model statistics (ps_kmer_stats) and the refits made from them ----------------------------------------------------
KMER_MAX_GROUPS = 256


def kmer_groups(events, groups=None, n_groups=None):
    """(group ids int32 [E], G) of a k-mer statistics call (PSAlign.KmerStats): `support_groups`' rules with up to 256 groups.
    `groups` defaults to the strand of every event (0 template, 1 complement, from ev.model.complement) and `n_groups` to 2 for
    that default, otherwise to the largest id + 1.  ValueError for a list that is not one id per event, G outside 1 .. 256 or an
    id outside 0 .. G - 1."""
    import numpy as np
    E = len(events)
    if groups is None:
        groups = [1 if getattr(ev.model, 'complement', False) else 0 for ev in events]
        if n_groups is None:
            n_groups = 2
    grp = np.asarray(list(groups), dtype=np.int64).reshape(-1)
    if grp.size != E:
        raise ValueError("kmer_stats: %d group ids for %d events" % (grp.size, E))
    G = int(n_groups) if n_groups is not None else (int(grp.max()) + 1 if E else 1)
    if not 1 <= G <= KMER_MAX_GROUPS:
        raise ValueError("kmer_stats: n_groups = %d, allowed are 1 .. %d" % (G, KMER_MAX_GROUPS))
    bad = np.flatnonzero((grp < 0) | (grp >= G))
    if bad.size:
        raise ValueError("kmer_stats: event %d has group %d, n_groups = %d" % (int(bad[0]), int(grp[bad[0]]), G))
    return grp.astype(np.int32), G


def model_lambda(sd_mean, sd_stdv):
    """sd_lambda = sd_mean^3 / sd_stdv^2 of every model row as the library's host tables hold it (pow of the C library, then one
    division; cpp/EventData.h:48-73)"""
    import numpy as np
    three, two = np.float64(3.0), np.float64(2.0)
    with np.errstate(all='ignore'):
        return np.array([np.float64(a) ** three / np.float64(b) ** two for a, b in zip(np.asarray(sd_mean, dtype=np.float64).reshape(-1).tolist(),
                                                                                       np.asarray(sd_stdv, dtype=np.float64).reshape(-1).tolist())], dtype=np.float64)


def kmer_stats_from_refs(states, events, refs, groups, n_groups):
    """The table of ps_kmer_stats (_capi.KMER_STATS [n_groups, 1024]) — the definition of include/poreseq_hip.h in numpy float64
    scalars, and the path of a library without the entry point.  states: the 5-mer states of the sequence (states[j - 1] belongs to
    column j); events: the event objects (mean, stdv and the model rows are read); refs: one ref_align array per event; groups:
    one id 0 .. n_groups - 1 per event.
    A level enters iff ra > 0, its column c = int(min(ra, 2147483647.0)) has 1 <= c <= len(states) and k = states[c - 1] lies in
    0 .. 1023 (ps_align_stats' n_fit rule).  With the event's rows m_k, s_k, mu_k = sd_mean[k], lam_k = sd_mean[k]^3 / sd_stdv[k]^2:
    z = (mean - m_k) / s_k, u = stdv / mu_k, p = lam_k / mu_k; n += 1, sz += z, szz += z z, sp += p, spu += p u, spv += p / u into
    table[group][k], every sum serial from 0.0: events in event order, levels ascending."""
    import numpy as np
    from ._capi import KMER_STATS
    states = np.asarray(states, dtype=np.int64).reshape(-1)
    S = states.size
    G = int(n_groups)
    n = np.zeros((G, 1024), dtype=np.int64)
    sums = np.zeros((5, G, 1024), dtype=np.float64)
    with np.errstate(all='ignore'):
        for ev, ra, g in zip(events, refs, np.asarray(groups).reshape(-1).tolist()):
            ra = np.asarray(ra, dtype=np.float64).reshape(-1)
            al = ra > 0
            col = np.zeros(ra.size, dtype=np.int64)
            col[al] = np.minimum(ra[al], 2147483647.0).astype(np.int64)
            has = al & (col >= 1) & (col <= S)
            k = np.full(ra.size, -1, dtype=np.int64)
            k[has] = states[col[has] - 1]
            idx = np.flatnonzero(has & (k >= 0) & (k < 1024))
            if not idx.size:
                continue
            md = ev.model
            lm, ls = np.asarray(md.level_mean, dtype=np.float64), np.asarray(md.level_stdv, dtype=np.float64)
            mu = np.asarray(md.sd_mean, dtype=np.float64)
            lam = model_lambda(mu, md.sd_stdv)
            kk = k[idx]
            z = (np.asarray(ev.mean, dtype=np.float64)[idx] - lm[kk]) / ls[kk]
            u = np.asarray(ev.stdv, dtype=np.float64)[idx] / mu[kk]
            p = lam[kk] / mu[kk]
            terms = (z, z * z, p, p * u, p / u)
            row = sums[:, g, :]
            for i, kq in enumerate(kk.tolist()):
                n[g, kq] += 1
                for q in range(5):
                    row[q, kq] = row[q, kq] + terms[q][i]
    table = np.zeros((G, 1024), dtype=KMER_STATS)
    table["n"] = n
    for q, name in enumerate(("sz", "szz", "sp", "spu", "spv")):
        table[name] = sums[q]
    return table


def add_kmer_stats(tables):
    """Pool k-mer tables of the same grouping (e.g. one per region of a lock-step batch): a host sum, field by field, in list
    order, starting from the first table.  Returns a new table."""
    import numpy as np
    tables = list(tables)
    if not tables:
        raise ValueError("add_kmer_stats: no tables")
    out = np.array(tables[0], copy=True)
    with np.errstate(all='ignore'):
        for t in tables[1:]:
            if t.shape != out.shape:
                raise ValueError("add_kmer_stats: tables of %r and %r" % (out.shape, t.shape))
            for name in out.dtype.names:
                out[name] = out[name] + t[name]
    return out


class KmerFit(object):
    """fit_kmers' result for one event group, arrays of 1024: n (levels), dmean (shift of level_mean in units of level_stdv), vscale
    (factor on level_stdv^2), sd_scale (factor on sd_mean), kept (identity: fewer than min_count levels or a non-finite term) and
    clamped (a limit cut the result)"""
    __slots__ = ("n", "dmean", "vscale", "sd_scale", "kept", "clamped")

    def __init__(self, n, dmean, vscale, sd_scale, kept, clamped):
        self.n, self.dmean, self.vscale, self.sd_scale, self.kept, self.clamped = n, dmean, vscale, sd_scale, kept, clamped

    @property
    def n_fitted(self):
        return int((~self.kept).sum())

    def __repr__(self):
        return "KmerFit(%d of 1024 k-mers fitted, %d clamped)" % (self.n_fitted, int(self.clamped.sum()))


def fit_kmers(table, prior=8.0, min_count=1, mean_limit=3.0, var_limits=(0.25, 4.0), sd_limits=(0.5, 2.0)):
    """Per-k-mer model refit from a ps_kmer_stats table [G, 1024] (or one row [1024]): one KmerFit per group (one KmerFit for a
    row).  With c = n / (n + prior), a shrinkage towards the model as it is (a k-mer seen `prior` times moves halfway):
        dmean = c sz / n;  vscale = 1 + c ((szz - sz sz / n) / n - 1);  sd_scale = 1 + c (spu / sp - 1)
    — the mean of the standardised residuals, their variance about that mean, and the maximiser of the inverse-Gaussian likelihood
    in a factor on sd_mean at fixed lambda.  A k-mer with n < max(min_count, 1) or a non-finite term keeps the identity (0, 1, 1) and
    is flagged `kept`; dmean is clamped to +-mean_limit, vscale to var_limits, sd_scale to sd_limits, flagged `clamped`.  The limits
    are guards with documented defaults, not measurements.  Host only."""
    import numpy as np
    table = np.asarray(table)
    if table.ndim == 2:
        return [fit_kmers(row, prior, min_count, mean_limit, var_limits, sd_limits) for row in table]
    n = table["n"].astype(np.int64)
    nf = n.astype(np.float64)
    with np.errstate(all='ignore'):
        c = nf / (nf + float(prior))
        mz = table["sz"] / nf
        dmean = c * mz
        vscale = 1.0 + c * ((table["szz"] - table["sz"] * table["sz"] / nf) / nf - 1.0)
        sd_scale = 1.0 + c * (table["spu"] / table["sp"] - 1.0)
        kept = (n < max(int(min_count), 1)) | ~(np.isfinite(dmean) & np.isfinite(vscale) & np.isfinite(sd_scale))
        for name in ("sz", "szz", "sp", "spu", "spv"):
            kept |= ~np.isfinite(table[name])
    dmean, vscale, sd_scale = np.where(kept, 0.0, dmean), np.where(kept, 1.0, vscale), np.where(kept, 1.0, sd_scale)
    lim = abs(float(mean_limit))
    cd, cv, cs = np.clip(dmean, -lim, lim), np.clip(vscale, var_limits[0], var_limits[1]), np.clip(sd_scale, sd_limits[0], sd_limits[1])
    clamped = (cd != dmean) | (cv != vscale) | (cs != sd_scale)
    return KmerFit(n, cd, cv, cs, kept, clamped)


class ScalingSdFit(tuple):
    """(a, D, ok, n) of fit_scaling_sd, with the fields by name"""
    __slots__ = ()
    _fields = ("a", "D", "ok", "n")

    def __new__(cls, a, D, ok, n):
        return tuple.__new__(cls, (float(a), float(D), bool(ok), int(n)))

    a = property(lambda self: self[0])
    D = property(lambda self: self[1])
    ok = property(lambda self: self[2])
    n = property(lambda self: self[3])

    def __repr__(self):
        return "ScalingSdFit(a=%r, D=%r, ok=%r, n=%r)" % tuple(self)


def fit_scaling_sd(table, min_levels=100, a_limits=(0.5, 2.0), var_limits=(0.25, 4.0)):
    """The stdv channel's scale_sd / var_sd refit of one event group, in closed form from the row sums of its ps_kmer_stats row
    [1024] (a table [G, 1024] gives a list, one fit per group).  The stdv of a level on state k is inverse Gaussian with mean mu_k
    and shape lam_k; its log-likelihood holds -0.5 lam (x - mu)^2 / (mu^2 x).  With a common factor a on every mu_k (lam_k
    fixed), u = x / mu_k and p = lam_k / mu_k that term is -0.5 p (u / a^2 - 2 / a + 1 / u), so
        a = sum spu / sum sp                                  the exact maximiser (d/da = 0), the scale_sd factor
        D = (sum spv - (sum sp)^2 / sum spu) / sum n          the mean deviance at a — 1 when the model is right — the var_sd
                                                              factor: the maximiser of a common factor 1 / D on every lam_k
    Returns ScalingSdFit(a, D, ok, n).  ok iff n >= min_levels and a, D are finite and inside their limits; a fit that is not ok is
    the identity (1, 1).  Host only; the limits are guards, not measurements."""
    import math
    import numpy as np
    table = np.asarray(table)
    if table.ndim == 2:
        return [fit_scaling_sd(row, min_levels, a_limits, var_limits) for row in table]
    n = int(table["n"].sum())
    with np.errstate(all='ignore'):
        sp, spu, spv = (float(np.sum(table[k])) for k in ("sp", "spu", "spv"))
    ident = ScalingSdFit(1.0, 1.0, False, n)
    if n < int(min_levels) or n <= 0 or not (sp > 0 and spu > 0):
        return ident
    a = spu / sp
    D = (spv - sp * sp / spu) / n
    if not (math.isfinite(a) and math.isfinite(D)) or not (a_limits[0] <= a <= a_limits[1] and var_limits[0] <= D <= var_limits[1]):
        return ident
    return ScalingSdFit(a, D, True, n)


def apply_kmers(event, fit):
    """Apply a KmerFit to an event's model in place (new arrays): level_mean += dmean * level_stdv, level_stdv *= sqrt(vscale) —
    the mean first: dmean is in units of the level_stdv the statistics were taken with — and sd_mean *= sd_scale.  sd_scale was
    fitted at fixed lambda = sd_mean^3 / sd_stdv^2, and the model stores sd_stdv, not lambda: sd_stdv *= sd_scale^1.5 keeps every
    lambda where it was.  Nothing else of the event is touched."""
    import numpy as np
    m = event.model
    ls = np.asarray(m.level_stdv, dtype=np.float64)
    m.level_mean = np.asarray(m.level_mean, dtype=np.float64) + fit.dmean * ls
    m.level_stdv = ls * np.sqrt(fit.vscale)
    m.sd_mean = np.asarray(m.sd_mean, dtype=np.float64) * fit.sd_scale
    m.sd_stdv = np.asarray(m.sd_stdv, dtype=np.float64) * fit.sd_scale ** 1.5
    return event


def apply_scaling_sd(event, a, D=1.0):
    """Apply fit_scaling_sd's (a, D) to an event's model in place (new arrays): sd_mean *= a, sd_stdv *= a^1.5 sqrt(D).
    The fit moves every mu to a mu and every lambda to lambda / D; the model stores sd_stdv with lambda = sd_mean^3 / sd_stdv^2, so
    sd_stdv'^2 = (a mu)^3 / (lambda / D) = a^3 D sd_stdv^2.  (A factor a sqrt(D) on sd_stdv would move lambda to a lambda / D, and
    a second fit would then answer D = a instead of 1.)  A second fit_scaling_sd after this gives a = 1, D = 1."""
    import numpy as np
    m = event.model
    m.sd_mean = np.asarray(m.sd_mean, dtype=np.float64) * float(a)
    m.sd_stdv = np.asarray(m.sd_stdv, dtype=np.float64) * (float(a) ** 1.5 * float(D) ** 0.5)
    return event


# ---- the backtrace's moves (ps_move_stats) and the transition rates fitted from them ---------------------------------------------
def moves_from_tables(main, stay, step_main, step_stay):
    """One event's backtrace, walked literally (cpp/Alignment.cpp:537-605) on the forward tables that `debug_fill` hands out —
    main / stay scores and their step codes, [levels + 1, states + 1], NaN outside the band — the definition of ps_move_stats in
    Python and the path of a library without the entry point.  The walk starts on the first maximum of the main scores that is
    > 0, columns before rows (the order the fill meets the cells in, cpp/Alignment.cpp:158, 270), and ends on row 0, on a score
    <= 0 or on a Z_IMPLICIT step.  Returns (record, step, col, ref_align, ref_like): the _capi.EVENT_MOVES record (shape (); `inert`
    is the caller's to set: the tables do not say whether the reference would have walked at all), per level the move code that
    recorded it (1 MATCH, 2 INSERT, 3 IGNORE, 4 STAY, 5 EXTEND, 0 off the path) and the column it was recorded on, and the
    ref_align / ref_like arrays the reference's backtrace writes.  Skips are counted step by step, a run ending at any other step."""
    import numpy as np
    from ._capi import EVENT_MOVES
    main, stay = np.asarray(main, dtype=np.float64), np.asarray(stay, dtype=np.float64)
    sm, ss = np.asarray(step_main), np.asarray(step_stay)
    n = main.shape[0] - 1
    rec = np.zeros((), dtype=EVENT_MOVES)
    step, col = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
    ra, rl = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    rec["n_levels"] = n
    # MaxInfo starts at (score 0, cell 0, 0) and moves on a strictly larger score only, column by column, rows ascending
    with np.errstate(invalid='ignore'):
        cand = np.where(main > 0, main, -np.inf).T      # [column, row]; NaN and scores <= 0 never win
    i = j = 0
    if cand.size and np.max(cand) > 0:
        j, i = np.unravel_index(int(np.argmax(cand)), cand.shape)   # (argmax: the first maximum in column-major order)
        i, j = int(i), int(j)
    rec["top_level"], rec["top_col"] = i, j
    counts = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0}
    run = runs = longest = skipped = 0
    arr = kind = 0

    def close_run():
        nonlocal run, runs, longest
        if run:
            runs += 1
            longest = max(longest, run)
        run = 0

    low = 0
    while i > 0:
        st = int((ss if arr else sm)[i, j])
        score = (stay if arr else main)[i, j]
        if np.isnan(score):
            raise ValueError("moves_from_tables: the walk left the band at level %d, column %d" % (i, j))
        if score <= 0.0:
            break
        if st == 0:                       # L_SKIP
            run += 1
            skipped += 1
            j -= 1
            continue
        close_run()
        if st == 4 and arr == 0:          # U_STAY on the main matrix: over to the stay matrix, same cell
            arr = 1
            continue
        if st not in counts:              # Z_IMPLICIT (or an unknown code): the walk ends here
            kind = 1 if st == 255 else 0
            break
        counts[st] += 1
        step[i - 1], col[i - 1] = st, j
        ra[i - 1] = -1.0 if st in (2, 3) else float(j)
        rl[i - 1] = score
        low = i
        if st == 4:
            arr = 0
        i -= 1
        if st in (1, 3):
            j -= 1
    close_run()
    rec["low_level"], rec["low_col"], rec["end_kind"] = low, j, kind
    rec["n_match"], rec["n_insert"], rec["n_ignore"], rec["n_stay"], rec["n_extend"] = counts[1], counts[2], counts[3], counts[4], counts[5]
    rec["n_skip_runs"], rec["max_skip"], rec["n_skip_cols"] = runs, longest, skipped
    return rec, step, col, ra, rl


TRANSITION_RATES = ("skip", "stay", "extend", "insert")


class TransitionFit(object):
    """fit_transitions' result: params (a copy of the given parameters with the fitted rates under 'skip_t' .. 'insert_c'), rates
    {key: value before the clamp}, counts {key: (numerator, denominator)} and flags {key: 'clamped' | 'empty'} for the rates that
    a limit cut or that had no observation (those keep the given value); logz: None, or — RefitTransitions(posterior=True) — the
    summed logz of all events before every round"""
    __slots__ = ("params", "rates", "counts", "flags", "logz")

    def __init__(self, params, rates, counts, flags):
        self.params, self.rates, self.counts, self.flags = params, rates, counts, flags
        self.logz = None

    @property
    def ok(self):
        return not self.flags

    def __repr__(self):
        return "TransitionFit(%s%s)" % (", ".join("%s=%.4g" % (k, self.params[k]) for k in sorted(self.rates)),
                                        "; flagged: " + ", ".join(sorted(self.flags)) if self.flags else "")


def fit_transitions(records, groups, params, prior=100.0, lo=1e-3, hi=0.5, suffixes=("_t", "_c")):
    """The transition probabilities of `params` re-estimated from ps_move_stats records (_capi.EVENT_MOVES [E]): the frequencies of
    the moves on the backtrace's paths, pooled per group — groups[e] is the group of record e, by default use the strand (0
    template, 1 complement), which gives the keys 'skip_t' .. 'insert_c' through `suffixes`.  With L = n_match + n_ignore +
    n_insert + n_stay + n_extend (the recorded levels) and Ccol = n_match + n_ignore + n_skip_cols (the columns the path crossed):
        skip = n_skip_cols / Ccol;  stay = n_stay / L;  extend = n_extend / (n_stay + n_extend);  insert = (n_insert + n_ignore) / L
    Each rate is shrunk towards the parameter as it is by `prior` pseudo-observations, (num + prior cur) / (den + prior), and
    clamped to [lo, hi]; a rate that was clamped is flagged 'clamped', one without an observation (denominator 0: an empty group,
    or no stay to extend) keeps the given value and is flagged 'empty' — fit_kmers' convention.  `lo`, `hi` and `prior` are guards
    with documented defaults, not measurements.  A key `params` lacks is taken from DEFAULT_PARAMS.
    These are path frequencies (Viterbi training) of a score that is no normalised probability (lik_offset is added per matched
    level), not maximum-likelihood estimates.  Host only.  Returns a TransitionFit."""
    import numpy as np
    return _fit_rates("fit_transitions", records, groups, params, prior, lo, hi, suffixes, _MOVE_FIELDS,
                      lambda col: int(np.sum(col, dtype=np.int64)))


# the six totals of a rate fit and the fields they are summed from: ps_event_moves' integers, ps_event_posterior's expectations
_FIT_TOTALS = ("n_match", "n_ignore", "n_insert", "n_stay", "n_extend", "n_skip_cols")
_MOVE_FIELDS = _FIT_TOTALS
_SOFT_FIELDS = ("e_match", "e_ignore", "e_insert", "e_stay", "e_extend", "e_skip")


def _fit_rates(who, records, groups, params, prior, lo, hi, suffixes, fields, total):
    """the one body of fit_transitions and fit_transitions_soft: `fields` names the six totals in the records, `total` sums one
    column of a group (to a Python int for counts, to a float for expectations)"""
    import numpy as np
    rec = np.asarray(records).reshape(-1)
    grp = np.asarray(list(groups), dtype=np.int64).reshape(-1)
    if grp.size != rec.size:
        raise ValueError("%s: %d group ids for %d records" % (who, grp.size, rec.size))
    if grp.size and (grp.min() < 0 or grp.max() >= len(suffixes)):
        raise ValueError("%s: group ids must lie in 0 .. %d" % (who, len(suffixes) - 1))
    if not (0.0 <= float(lo) <= float(hi)) or float(prior) < 0:
        raise ValueError("%s: need 0 <= lo <= hi and prior >= 0" % who)
    out, rates, counts, flags = dict(params), {}, {}, {}
    for g, suf in enumerate(suffixes):
        r = rec[grp == g]
        tot = {k: total(r[f]) for k, f in zip(_FIT_TOTALS, fields)}
        L = tot["n_match"] + tot["n_ignore"] + tot["n_insert"] + tot["n_stay"] + tot["n_extend"]
        ccol = tot["n_match"] + tot["n_ignore"] + tot["n_skip_cols"]
        frac = {"skip": (tot["n_skip_cols"], ccol), "stay": (tot["n_stay"], L), "extend": (tot["n_extend"], tot["n_stay"] + tot["n_extend"]),
                "insert": (tot["n_insert"] + tot["n_ignore"], L)}
        for name in TRANSITION_RATES:
            key = name + suf
            cur = float(params[key]) if key in params else float(DEFAULT_PARAMS[key])
            num, den = frac[name]
            counts[key] = (num, den)
            if den <= 0:
                rates[key], out[key], flags[key] = cur, cur, 'empty'
                continue
            v = (num + float(prior) * cur) / (den + float(prior))
            rates[key] = v
            out[key] = min(max(v, float(lo)), float(hi))
            if out[key] != v:
                flags[key] = 'clamped'
    return TransitionFit(out, rates, counts, flags)


def fit_transitions_soft(records, groups, params, prior=100.0, lo=1e-3, hi=0.5, suffixes=("_t", "_c")):
    """fit_transitions on EXPECTED move counts: `records` are ps_posterior_stats records (_capi.EVENT_POSTERIOR [E]), whose e_skip ..
    e_extend are the expected numbers of each move under the sum over all alignments in the band (posterior_from_emissions).  The
    formulas, the shrinkage by `prior`, the clamps and the flags are fit_transitions' own (one body, _fit_rates), with e_match,
    e_ignore, e_insert, e_stay, e_extend in the places of the n_ fields and e_skip in that of n_skip_cols:
        skip = e_skip / (e_match + e_ignore + e_skip);  stay = e_stay / L;  extend = e_extend / (e_stay + e_extend);
        insert = (e_insert + e_ignore) / L,   L = e_match + e_ignore + e_insert + e_stay + e_extend
    Totals are summed with math.fsum (correctly rounded, whatever the order of the records).  On integer-valued expectations the result is fit_transitions'.  One round of
    a Baum-Welch-like re-estimation of a score that is no normalised probability (the floor terms and lik_offset), not a
    maximum-likelihood estimate; what it does to consensus accuracy on real data has not been measured.  Host only."""
    import math
    return _fit_rates("fit_transitions_soft", records, groups, params, prior, lo, hi, suffixes, _SOFT_FIELDS,
                      lambda col: math.fsum(float(v) for v in col))


def strand_groups(events):
    """the default grouping of fit_transitions: 0 for a template event, 1 for a complement one (ev.model.complement)"""
    return [1 if getattr(ev.model, 'complement', False) else 0 for ev in events]


# ---- posterior move counts: the sum over all alignments in the band (ps_posterior_stats) ------------------------------------------
LOG2PI = 1.8378770664093453      # log(2 pi) as the library forms it (cpp/AlignUtil.h:24)
REF_INF = 1e300                   # the reference's "inf" (cpp/AlignUtil.h:20): the floor of a band's first stay cell in 'max' mode


class Posterior(object):
    """posterior_from_emissions' result.  logz (sum mode; the best score in 'max' mode), counts {e_skip, e_match, e_ignore, e_insert,
    e_stay, e_extend} (sum mode), n_cells / n_cols (band cells of the columns with a state, and those columns), main / stay (the
    forward tables [n0 + 1][C + 1], NaN outside the band, 0 in the blank column and in columns without a state), emit / col (per
    level, when asked for)"""
    __slots__ = ("logz", "counts", "n_cells", "n_cols", "main", "stay", "emit", "col")

    def record(self, n_levels, inert=0):
        """the _capi.EVENT_POSTERIOR record of this result (float64)"""
        import numpy as np
        from ._capi import EVENT_POSTERIOR
        r = np.zeros((), dtype=EVENT_POSTERIOR)
        r["n_levels"], r["inert"], r["n_cols"], r["n_cells"], r["logz"] = n_levels, inert, self.n_cols, self.n_cells, float(self.logz)
        for k, v in self.counts.items():
            r[k] = float(v)
        return r


def fill_emissions(event, states, params):
    """obs [n0 + 1][C + 1] float64: the forward fill's emission of every level of `event` against every state of `states` (row 0,
    column 0 and the columns without a state: 0), operation for operation as the library forms it (cpp/AlignUtil.h:34-53,
    cpp/Alignment.cpp:169-173): logarithms and pow(., 3) through libm, lambda = pow(sd_mean, 3) / (sd_stdv * sd_stdv), the level's
    log stdv MIRRORED — row i takes 3 log(stdv[n0 - i]), sic — and lik_offset added last."""
    import math
    import numpy as np
    m = event.model
    lm, ls = np.asarray(m.level_mean, dtype=np.float64), np.asarray(m.level_stdv, dtype=np.float64)
    sm, ss = np.asarray(m.sd_mean, dtype=np.float64), np.asarray(m.sd_stdv, dtype=np.float64)
    with np.errstate(all='ignore'):
        lam = np.array([math.pow(a, 3) / (b * b) if b != 0 else float('nan') for a, b in zip(sm.tolist(), ss.tolist())])
        log_lev = np.array([math.log(x) if x > 0 else float('nan') for x in ls.tolist()])
        log_lam = np.array([math.log(x) if x > 0 else float('nan') for x in lam.tolist()])
    mean, stdv = np.asarray(event.mean, dtype=np.float64), np.asarray(event.stdv, dtype=np.float64)
    n0 = mean.size
    st = np.asarray(states, dtype=np.int64).reshape(-1)
    C = st.size
    obs = np.zeros((n0 + 1, C + 1))
    ok = np.nonzero(st >= 0)[0]
    if not n0 or not ok.size:
        return obs
    k = st[ok]
    lsd3 = 3.0 * np.array([math.log(x) if x > 0 else float('nan') for x in stdv.tolist()])[::-1]      # row i: 3 log stdv[n0 - i]
    off = float(params.get('lik_offset', DEFAULT_PARAMS['lik_offset']))
    with np.errstate(all='ignore'):
        d = (mean[:, None] - lm[k][None, :]) / ls[k][None, :]
        l = -0.5 * (d * d + LOG2PI) - log_lev[k][None, :]
        e = (stdv[:, None] - sm[k][None, :]) / sm[k][None, :]
        q = (e * e * lam[k][None, :]) / stdv[:, None]
        g = 0.5 * (log_lam[k][None, :] - lsd3[:, None] - LOG2PI - q)
        l = l + g
        l = l + off
    obs[1:, ok + 1] = l
    return obs


def posterior_from_emissions(obs, mask, valid, lik_skip, lik_stay, lik_extend, lik_insert, semiring='sum', dtype=None, levels=False, counts=True):
    """The sum-product (or, semiring='max', the reference's max-plus) fill of one event's band, and the expected move counts under
    it: the definition of ps_posterior_stats (include/poreseq_hip.h) in numpy.
      obs    [n0 + 1][C + 1] emissions (fill_emissions); read inside the band of the columns with a state only
      mask   [n0 + 1][C + 1] bool: the cells the forward fill holds — column 0 the blank column, rows 0 .. n0; column j the rows
             i0(j) .. i1(j) (the non-NaN pattern of debug_fill, direction 0)
      valid  [C + 1] bool: column j has a 5-mer state (valid[0] is ignored: the blank column has none)
      lik_*  the four log transition probabilities
    The recursion is cpp/Alignment.cpp:189-267 with (+) = log-sum-exp in place of every max ('max': max).  A column without a state
    and the blank column hold M = S = 0 on their rows, constants through which nothing flows.  In a column with a state, with the
    previous column's band p0 .. p1 and Mp its M (0 where the text says "implicit"):
      S(i, j) = 0 (+) (M(i-1, j) + obs + lik_stay) (+) (S(i-1, j) + obs + lik_extend)   for i > i0;   S(i0, j) = -inf ('max': -1e300)
      M(i, j) = 0 (+) skip (+) match (+) ignore (+) insert (+) S(i, j)
      skip = Mp(i) + lik_skip (Mp = 0 unless p0 <= i <= p1);  match = Mp(i-1) + obs (Mp = 0 unless p0 < i <= p1);
      ignore = Mp(i-1) + lik_insert, only when p0 < i <= p1;  insert = M(i-1, j) + lik_insert, only when i > i0
      logz = (+) of M over the band cells of the columns with a state (0 when there is none)
    The expected count of a move is the sum over cells of exp(F(pred) + w + beta(cell) - logz), F(pred) = 0 for a constant or
    implicit predecessor, beta the backward quantity of the same lattice: beta_M(c) = 0 (the path ends here) (+) every move out of
    M(c), beta_S(c) = beta_M(c) (+) the extend out of S(c).  With levels=True, emit[i-1] is the expected number of emitting arrivals
    (match + stay + extend) at level i and col[i-1] their posterior mean column (NaN where emit is 0).
    Cells of one anti-diagonal do not depend on each other; the recursion runs over anti-diagonals, vectorised along each.
    dtype: numpy float64 (default) or longdouble.  counts=False stops after logz (no backward pass; counts stay 0).  Returns a
    Posterior."""
    import numpy as np
    ft = np.dtype(np.float64 if dtype is None else dtype).type
    if semiring not in ('sum', 'max'):
        raise ValueError("posterior_from_emissions: semiring must be 'sum' or 'max'")
    mask = np.asarray(mask, dtype=bool)
    n0, C = mask.shape[0] - 1, mask.shape[1] - 1
    ok = np.asarray(valid, dtype=bool).reshape(-1).copy()
    if ok.size != C + 1 or np.asarray(obs).shape != mask.shape:
        raise ValueError("posterior_from_emissions: shapes of obs, mask and valid do not fit")
    ok[0] = False
    NINF = ft(-np.inf)
    lsk, lst, lex, lin = ft(lik_skip), ft(lik_stay), ft(lik_extend), ft(lik_insert)
    # everything padded by one row and one column on the far side, so that (i + 1, j + 1) always exists
    mk = np.zeros((n0 + 2, C + 2), dtype=bool)
    mk[:n0 + 1, :C + 1] = mask
    live = mk.copy()
    live[:, :C + 1] &= ok[None, :]
    live[:, 0] = False
    o = np.zeros((n0 + 2, C + 2), dtype=ft)
    with np.errstate(invalid='ignore'):
        o[:n0 + 1, :C + 1] = np.where(live[:n0 + 1, :C + 1], np.asarray(obs), 0.0)
    FM = np.zeros((n0 + 2, C + 2), dtype=ft)      # read as Mp: 0 outside the band and in the constant columns
    FS = np.zeros((n0 + 2, C + 2), dtype=ft)

    def lse(terms):
        t = np.stack(terms)
        if semiring == 'max':
            return np.max(t, axis=0)
        m = np.max(t, axis=0)
        with np.errstate(invalid='ignore'):
            return m + np.log(np.sum(np.exp(t - m[None, :]), axis=0))

    ci, cj = np.nonzero(live)
    order = np.argsort(ci + cj, kind='stable')
    ci, cj = ci[order], cj[order]
    cuts = np.nonzero(np.diff(ci + cj))[0] + 1
    diags = list(zip(np.split(ci, cuts), np.split(cj, cuts))) if ci.size else []
    up_ok = np.zeros_like(mk)
    up_ok[1:, :] = mk[:-1, :]
    up_ok &= live                                   # i > i0: the cell above is in the column's band
    dg_ok = np.zeros_like(mk)
    dg_ok[1:, 1:] = mk[1:, :-1] & mk[:-1, :-1]      # p0 < i <= p1
    dg_ok &= live
    top_floor = ft(-REF_INF) if semiring == 'max' else NINF
    zero = ft(0.0)
    for ii, jj in diags:
        ob = o[ii, jj]
        u, d = up_ok[ii, jj], dg_ok[ii, jj]
        D = np.where(d, FM[ii - 1, jj - 1], zero)
        um, us = FM[ii - 1, jj], FS[ii - 1, jj]
        z = np.zeros(ii.size, dtype=ft)
        s_in = lse([z, np.where(u, um + ob + lst, NINF), np.where(u, us + ob + lex, NINF)])
        S = np.where(u, s_in, top_floor)
        M = lse([z, FM[ii, jj - 1] + lsk, D + ob, np.where(d, D + lin, NINF), np.where(u, um + lin, NINF), S])
        FM[ii, jj], FS[ii, jj] = M, S
    res = Posterior()
    nan = ft(np.nan)
    res.main = np.where(mask, FM[:n0 + 1, :C + 1], nan)
    res.stay = np.where(mask, FS[:n0 + 1, :C + 1], nan)
    res.n_cells = int(ci.size)
    res.n_cols = int(np.count_nonzero(np.any(live, axis=0)))
    res.counts = dict.fromkeys(("e_skip", "e_match", "e_ignore", "e_insert", "e_stay", "e_extend"), ft(0.0))
    res.emit = res.col = None
    if levels:
        res.emit, res.col = np.zeros(n0, dtype=ft), np.full(n0, nan, dtype=ft)
    if not ci.size:
        res.logz = ft(0.0)
        return res
    cells = FM[ci, cj]
    if semiring == 'max':
        res.logz = max(ft(0.0), np.max(cells))
        return res
    top = np.max(cells)
    logz = top + np.log(np.sum(np.exp(cells - top)))
    res.logz = logz
    if not counts:
        return res
    # backward: beta over descending anti-diagonals; -inf wherever nothing flows (outside the band, constant columns)
    BM = np.full((n0 + 2, C + 2), NINF, dtype=ft)
    BS = np.full((n0 + 2, C + 2), NINF, dtype=ft)
    for ii, jj in reversed(diags):
        dn = mk[ii + 1, jj]                          # i + 1 <= i1(j): the match / ignore into (i + 1, j + 1) reads this cell, not the implicit 0
        bd = BM[ii + 1, jj + 1]
        z = np.zeros(ii.size, dtype=ft)
        bm = lse([z, BM[ii, jj + 1] + lsk, np.where(dn, bd + o[ii + 1, jj + 1], NINF), np.where(dn, bd + lin, NINF),
                  BM[ii + 1, jj] + lin, BS[ii + 1, jj] + o[ii + 1, jj] + lst])
        BM[ii, jj] = bm
        BS[ii, jj] = lse([bm, BS[ii + 1, jj] + o[ii + 1, jj] + lex])
    ob, bM, bS = o[ci, cj], BM[ci, cj] - logz, BS[ci, cj] - logz
    u, d = up_ok[ci, cj], dg_ok[ci, cj]
    D = np.where(d, FM[ci - 1, cj - 1], zero)
    with np.errstate(invalid='ignore'):
        w_skip = np.exp(FM[ci, cj - 1] + lsk + bM)
        w_match = np.exp(D + ob + bM)
        w_ign = np.where(d, np.exp(D + lin + bM), zero)
        w_ins = np.where(u, np.exp(FM[ci - 1, cj] + lin + bM), zero)
        w_stay = np.where(u, np.exp(FM[ci - 1, cj] + ob + lst + bS), zero)
        w_ext = np.where(u, np.exp(FS[ci - 1, cj] + ob + lex + bS), zero)
    res.counts = {"e_skip": np.sum(w_skip), "e_match": np.sum(w_match), "e_ignore": np.sum(w_ign), "e_insert": np.sum(w_ins),
                  "e_stay": np.sum(w_stay), "e_extend": np.sum(w_ext)}
    if levels:
        w = w_match + w_stay + w_ext
        emit = np.zeros(n0 + 2, dtype=ft)
        colw = np.zeros(n0 + 2, dtype=ft)
        np.add.at(emit, ci, w)
        np.add.at(colw, ci, w * cj.astype(ft))
        with np.errstate(invalid='ignore', divide='ignore'):
            res.emit, res.col = emit[1:n0 + 1], np.where(emit[1:n0 + 1] > 0, colw[1:n0 + 1] / emit[1:n0 + 1], nan)
    return res
