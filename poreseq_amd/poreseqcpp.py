"""Drop-in for the reference's compiled module `poreseq.poreseqcpp` (poreseq/_poreseqcpp.pyx).

Same names, argument meaning, return types and in-place behaviour: `PSAlign`, `swalign`,
`seqtostates`.  Where the reference's Cython code calls its C++ core, this module calls
the C ABI of include/poreseq_hip.h, served by hand-written HIP kernels
(poreseq_amd/csrc).  There is no CPU path: importing works anywhere, but every compute
call raises if libporeseq_hip.so is missing or no MI355X-class device is usable.
"""
import copy
import math

import numpy as np

from . import _capi
from .util import MutationInfo, MutationScore, support_groups, spans_from_refs, support_from_deltas, genotypes_from_deltas, check_alt_frac, phase_from_deltas, check_phase_args
from .util import align_stats_from_refs, fit_scaling, apply_scaling
from .util import kmer_groups, kmer_stats_from_refs, fit_kmers, apply_kmers
from .util import moves_from_tables, fit_transitions, strand_groups
from .util import fill_emissions, posterior_from_emissions, fit_transitions_soft


def _api():
    return _capi.load_hip()


def swalign(seq1, seq2, _api=_api):
    """Smith-Waterman align two sequences (pyx:155-174).

    Returns (accuracy in %, [(i1, i2), ...]) with 1-based indices and 0 for a gap.
    """
    _score, acc, i1, i2 = _api().swfull(seq1, seq2)
    return (acc, list(zip(i1.tolist(), i2.tolist())))


def swalign_summaries(pairs, _api=_api):
    """Smith-Waterman of every (seq1, seq2) pair in ONE batched call, each reduced to a `_capi.SwSummary`: what the consensus
    driver reads off swalign's list (Mutate.py:59-68, 93-98) — first and last aligned pair, gap counts, identity — without the
    list.  Identical pairs are aligned once (the replicas of `train` share reads and draft).  Returns the records in the order of `pairs`.
    """
    pairs = [(a, b) for a, b in pairs]
    slot = {}
    for p in pairs:
        slot.setdefault(p, len(slot))
    res = _api().sw_summaries(list(slot))
    return [res[slot[p]] for p in pairs]


def seqtostates(seq, _api=_api):
    """5-mer states [0, 1023] of a nucleotide string (pyx:176-187)."""
    return _api().seq_to_states(seq).tolist()


def _check_realign_accuracy(acc):
    if np.any(np.asarray(acc) < 0.6):  # sic: compares a percentage, as the reference does (pyx:256)
        raise Exception('Error rate too large for realignment!')


def point_table_from_list(n, start, orig, mut, score):
    """The point-edit table of a scored FindPointMutations list, built literally — the definition of what ps_point_table returns:
    every edit goes to row `start`, slot 0 for a deletion (mut == ''), 1 + 'ACGT'.index(mut) for a substitution, 5 + that for an
    insertion (orig == ''); slots without an edit (the substitution by the base itself) stay NaN.  margin / slot come from numpy's
    argmax (the first maximum) over the row with NaN masked, n_positive counts the entries > 0.
    Returns (table float64 [n, 9], margin float64 [n], slot int32 [n], n_positive int32 [n])."""
    table = np.full((int(n), _capi.POINT_SLOTS), np.nan, dtype=np.float64)
    for p, o, m, sc in zip(start, orig, mut, score):
        table[int(p), 0 if m == '' else ('ACGT'.index(m) + (5 if o == '' else 1))] = sc
    slot = np.argmax(np.where(np.isnan(table), -np.inf, table), axis=1).astype(np.int32)
    margin = table[np.arange(int(n)), slot]
    return table, margin, slot, np.sum(table > 0, axis=1).astype(np.int32)


def _scored_list(start, orig, mut, score):
    out = []
    for i in range(len(start)):
        s = MutationScore()
        s.start = int(start[i])
        s.orig = orig[i]
        s.mut = mut[i]
        s.score = float(score[i])
        out.append(s)
    return out


def _support_on(api, h, hm, n_events, seq_len, grp, G):
    """(scores, support, scored list) of the edit list `hm` on the AlignData `h`: ps_score_mutation_support, or — a library without
    the entry point — the literal reduction of its score_mutation_deltas and of the refs it leaves (util.support_from_deltas)"""
    start, orig, mut, _ = api.muts_export(hm)
    if "ps_score_mutation_support" in api.missing:
        deltas = api.score_mutation_deltas(h, hm, n_events, len(start))
        spans = spans_from_refs(api.align_event_refs(h, n_events))
        scores, sup = support_from_deltas(deltas, grp, G, spans, start, seq_len)
    else:
        scores, sup = api.score_mutation_support(h, hm, len(start), grp, G)
    return scores, sup, _scored_list(start, orig, mut, scores)


def _genotypes_on(api, h, hm, n_events, seq_len, grp, G, frac):
    """(scores, support, scored list, lik, n_cover) of the edit list `hm` on the AlignData `h`: ps_score_mutation_genotypes, or — a
    library without the entry point — the literal reductions of its score_mutation_deltas and of the refs it leaves
    (util.support_from_deltas, util.genotypes_from_deltas)"""
    start, orig, mut, _ = api.muts_export(hm)
    if "ps_score_mutation_genotypes" in api.missing:
        deltas = api.score_mutation_deltas(h, hm, n_events, len(start))
        spans = spans_from_refs(api.align_event_refs(h, n_events))
        scores, sup = support_from_deltas(deltas, grp, G, spans, start, seq_len)
        lik, n_cover = genotypes_from_deltas(deltas, spans, start, seq_len, frac)
    else:
        scores, sup, lik, n_cover = api.score_mutation_genotypes(h, hm, len(start), grp, G, frac)
    return scores, sup, _scored_list(start, orig, mut, scores), lik, n_cover


def _phase_on(api, h, hm, n_events, seq_len, window, min_link, max_sets):
    """(scores, link, phase, hap, n_sets, scored list) of the site list `hm` on the AlignData `h`: ps_score_mutation_phase, or — a
    library without the entry point — the literal reductions of its score_mutation_deltas and of the refs it leaves
    (util.phase_from_deltas; the scores are support_from_deltas')"""
    start, orig, mut, _ = api.muts_export(hm)
    if "ps_score_mutation_phase" in api.missing:
        deltas = api.score_mutation_deltas(h, hm, n_events, len(start))
        spans = spans_from_refs(api.align_event_refs(h, n_events))
        scores, _ = support_from_deltas(deltas, np.zeros(n_events, dtype=np.int32), 1, spans, start, seq_len)
        link, phase, hap, n_sets = phase_from_deltas(deltas, spans, start, seq_len, window, min_link, max_sets)
    else:
        scores, link, phase, hap, n_sets = api.score_mutation_phase(h, hm, len(start), n_events, window, min_link, max_sets)
    return scores, link, phase, hap, n_sets, _scored_list(start, orig, mut, scores)


def _align_stats_on(api, h, events, realign):
    """(scores float64 [E] or None, stats _capi.EVENT_STATS [E]) of the AlignData `h`, whose events are `events`: ps_align_stats,
    or — a library without the entry point — its score_alignments (with `realign`) and then the literal reduction of the refs the
    handle holds (util.align_stats_from_refs)"""
    E = len(events)
    if "ps_align_stats" not in api.missing:
        return api.align_stats(h, E, realign)
    scores = api.score_alignments(h, E) if realign else None
    refs = api.align_event_refs(h, E)
    states = api.seq_to_states(api.align_sequence(h))
    stats = np.zeros(E, dtype=_capi.EVENT_STATS)
    for e, ev in enumerate(events):
        stats[e] = align_stats_from_refs(states, ev.mean, refs[e], ev.model.level_mean, ev.model.level_stdv)
    return scores, stats


def _recalibrate(events, stats, var, fit_kw):
    """fit_scaling of every record, applied to the models of the events whose fit is ok -> the fits"""
    fits = fit_scaling(stats, **fit_kw)
    for ev, f in zip(events, fits):
        if f.ok:
            apply_scaling(ev, f, var=var)
    return fits


def _kmer_stats_on(api, h, events, grp, G, realign):
    """(scores float64 [E] or None, table _capi.KMER_STATS [G, 1024]) of the AlignData `h`, whose events are `events`: ps_kmer_stats,
    or — a library without the entry point — its score_alignments (with `realign`) and then the literal reduction of the refs the
    handle holds (util.kmer_stats_from_refs)"""
    E = len(events)
    if "ps_kmer_stats" not in api.missing:
        return api.kmer_stats(h, E, grp, G, realign)
    scores = api.score_alignments(h, E) if realign else None
    refs = api.align_event_refs(h, E)
    states = api.seq_to_states(api.align_sequence(h))
    return scores, kmer_stats_from_refs(states, events, refs, grp, G)


def _move_stats_on(api, h, events, params, levels):
    """(scores float64 [E], records _capi.EVENT_MOVES [E][, step, col]) of the AlignData `h`, whose events are `events` and whose
    parameters `params`: ps_move_stats, or — a library without the entry point — the literal walk (util.moves_from_tables) of the
    forward tables its debug_fill hands out, taken on a scratch AlignData with the sequence and the ref_align that `h` holds (a
    checker's debug_fill backtraces into the handle it is given), and then
    its score_alignments on `h`, which leaves the refs a scoring call leaves.  An event the reference would not walk
    (realign_width 0, or no aligned level) gets the inert record."""
    E = len(events)
    nl = [len(ev.mean) for ev in events]
    if "ps_move_stats" not in api.missing:
        return api.move_stats(h, nl, levels)
    recs = np.zeros(E, dtype=_capi.EVENT_MOVES)
    step = [np.zeros(n, dtype=np.uint8) for n in nl]
    col = [np.zeros(n, dtype=np.int32) for n in nl]
    sequence = api.align_sequence(h)                  # (what the handle holds now: a resident one may be ahead of the Python objects)
    S = len(api.seq_to_states(sequence))
    width = int(params.get('realign_width', 300))      # (cpp/AlignUtil.h:64: the default of a call that sets none)
    held = []
    for ev, ra in zip(events, api.align_event_refs(h, E)):
        ev = copy.copy(ev)
        ev.ref_align = ra
        held.append(ev)
    scratch = api.align_create(sequence, held, params)
    try:
        for e, ev in enumerate(held):
            recs[e]["n_levels"] = nl[e]
            with np.errstate(invalid='ignore'):
                walks = width != 0 and bool(np.any(ev.ref_align > 0))
            if not walks:
                recs[e]["inert"] = 1
                continue
            recs[e], step[e], col[e], _, _ = moves_from_tables(*api.debug_fill(scratch, e, 0, nl[e], S))
    finally:
        api.align_destroy(scratch)
    scores = api.score_alignments(h, E)
    return (scores, recs, step, col) if levels else (scores, recs)


def _posterior_stats_on(api, h, events, params, levels):
    """records _capi.EVENT_POSTERIOR [E] (levels: (records, emit, col)) of the AlignData `h`, whose events are `events` and whose
    parameters `params`: ps_posterior_stats, or — a library without the entry point — the definition itself,
    util.posterior_from_emissions, on util.fill_emissions and the band pattern of the forward tables the library's debug_fill hands
    out, taken on a scratch AlignData with the sequence and the ref_align that `h` holds.  `h` is not touched.  An event the
    reference would not fill (realign_width 0, no aligned level, no level) gets the inert record."""
    E = len(events)
    nl = [len(ev.mean) for ev in events]
    if "ps_posterior_stats" not in api.missing:
        return api.posterior_stats(h, nl, levels)
    recs = np.zeros(E, dtype=_capi.EVENT_POSTERIOR)
    emit = [np.zeros(n) for n in nl]
    col = [np.full(n, np.nan) for n in nl]
    sequence = api.align_sequence(h)
    states = api.seq_to_states(sequence)
    valid = np.concatenate([[False], np.asarray(states) >= 0])
    width = int(params.get('realign_width', 300))
    held = []
    for ev, ra in zip(events, api.align_event_refs(h, E)):
        ev = copy.copy(ev)
        ev.ref_align = ra
        held.append(ev)
    scratch = api.align_create(sequence, held, params)
    try:
        for e, ev in enumerate(held):
            recs[e]["n_levels"] = nl[e]
            with np.errstate(invalid='ignore'):
                fills = width != 0 and nl[e] > 0 and bool(np.any(ev.ref_align > 0))
            if not fills:
                recs[e]["inert"] = 1
                continue
            mask = ~np.isnan(api.debug_fill(scratch, e, 0, nl[e], len(states))[0])
            lik = [math.log(float(getattr(ev.model, 'prob_' + r))) for r in ("skip", "stay", "extend", "insert")]
            res = posterior_from_emissions(fill_emissions(ev, states, params), mask, valid, *lik, levels=levels)
            recs[e] = res.record(nl[e])
            if levels:
                emit[e], col[e] = np.asarray(res.emit, dtype=np.float64), np.asarray(res.col, dtype=np.float64)
    finally:
        api.align_destroy(scratch)
    return (recs, emit, col) if levels else recs


def _refit_transitions(events, records, groups, params, fit_kw, soft=False):
    """util.fit_transitions (soft: util.fit_transitions_soft) of the records, applied through PSEvent.setparams to every event ->
    the fit"""
    base = dict(params) if params is not None else {}
    for ev, g in zip(events, groups):      # the rates the events carry now, where `params` does not say
        for name in ("skip", "stay", "extend", "insert"):
            base.setdefault(name + ("_c" if g else "_t"), float(getattr(ev.model, 'prob_' + name)))
    fit = (fit_transitions_soft if soft else fit_transitions)(records, groups, base, **fit_kw)
    keys = {k: fit.params[k] for k in fit.rates}
    for ev in events:
        ev.setparams(keys)
    return fit


def _refit_posterior(stats, events_per_region, params, iters, fit_kw):
    """`iters` rounds of {stats() -> one EVENT_POSTERIOR array per region, util.fit_transitions_soft pooled over the regions per
    strand, setparams on every event}: round k starts from the rates round k - 1 set.  -> the last fit, with `logz`: the summed
    logz before every round"""
    if int(iters) < 1:
        raise ValueError("RefitTransitions(posterior=True): iters must be >= 1")
    events = [ev for evs in events_per_region for ev in evs]
    groups = strand_groups(events)
    cur, logz, fit = params, [], None
    for _ in range(int(iters)):
        records = np.concatenate(stats())
        logz.append(math.fsum(float(v) for v in records["logz"]))
        fit = _refit_transitions(events, records, groups, cur, fit_kw, soft=True)
        cur = fit.params
    fit.logz = logz
    return fit


def _refit_kmers(events, grp, fits):
    """apply_kmers of every event's group's fit, in place on the events' models -> the events whose model changed"""
    changed, seen = 0, set()
    for ev, g in zip(events, np.asarray(grp).tolist()):
        f = fits[g]
        if f.n_fitted:
            if id(ev.model) not in seen:      # (a model object shared by several events is refitted once)
                seen.add(id(ev.model))
                apply_kmers(ev, f)
            changed += 1
    return changed


class PSAlign:
    """All data of reads aligned to a reference (pyx:189-472).

    Attributes:
        sequence (str): the sequence the events are currently aligned to
        events (list): event objects (see poreseq_amd.events.PSEvent for the duck type)
        params (dict): 'verbose', 'lik_offset', 'realign_width', 'scoring_width', 'point_width'
    All methods work in place; use .Copy() first for non-destructive behaviour.
    """

    _native = staticmethod(_api)  # tests rebind this to the oracle / reference shim

    def __init__(self):
        self.sequence = ""
        self.events = []
        self.params = {}

    # -- plumbing ---------------------------------------------------------------
    class _Data:
        """Scoped native AlignData built from `self`, as PythonToAlignData does per call (pyx:139-153)."""

        def __init__(self, pa, point_width=False):
            self.api = pa._native()
            self.h = self.api.align_create(pa.sequence, pa.events, pa.params)
            if point_width and 'point_width' in pa.params:
                self.api.check(self.api.lib.ps_align_set_scoring_width(self.h, int(pa.params['point_width'])))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.api.align_destroy(self.h)
            return False

    def _scores_to_py(self, api, hm):
        start, orig, mut, score = api.muts_export(hm)
        out = []
        for i in range(len(start)):
            s = MutationScore()
            s.start = int(start[i])
            s.orig = orig[i]
            s.mut = mut[i]
            s.score = float(score[i])
            out.append(s)
        return out

    # -- reference API ----------------------------------------------------------
    def Copy(self):
        return copy.deepcopy(self)

    def Coverage(self):
        """Events aligned over each base of self.sequence (pyx:225-239)."""
        cov = np.zeros(len(self.sequence))
        for ev in self.events:
            nzs = ev.ref_align[ev.ref_align > 0]
            lo = int(nzs[0])
            hi = int(np.minimum(nzs[-1], len(cov) - 1))
            cov[lo:hi] += 1
        return cov

    def RealignTo(self, newseq):
        """Re-map every event onto `newseq` through swalign (pyx:241-261)."""
        align = swalign(self.sequence, newseq, self._native)
        if align[0] < 0.6:  # sic: compares a percentage, as the reference does (pyx:256)
            raise Exception('Error rate too large for realignment!')
        pairs = np.array(align[1])
        for ev in self.events:
            ev.mapaligns(pairs)
        self.sequence = newseq

    def ScoreEvents(self):
        """Total likelihood score of each event (pyx:263-276).  Does not write ref_align back."""
        with PSAlign._Data(self) as d:
            return d.api.score_alignments(d.h, len(self.events)).tolist()

    def AlignStats(self, realign=True):
        """Per event the census of its alignment and the sums of a shift / scale refit of its model (ps_align_stats): (scores,
        stats).  realign=True aligns every event as ScoreEvents does — scores are ScoreEvents' bits, as float64 [E] — and reduces the
        alignment that leaves, on the device, in the same launch chain (k_align_stats); realign=False reduces ref_align as the
        events carry it, runs no DP and returns None for the scores.  stats is a structured array (_capi.EVENT_STATS [E]): the
        levels by kind, the steps between consecutive aligned levels by size, and sw .. swrr for util.fit_scaling.  Like
        ScoreEvents it does not write ref_align back; `self` is not modified."""
        with PSAlign._Data(self) as d:
            return _align_stats_on(d.api, d.h, self.events, bool(realign))

    def Recalibrate(self, var=True, **fit_kw):
        """Refit every event's model scaling on its alignment to self.sequence: one AlignStats() pass, util.fit_scaling(**fit_kw) per
        event, and util.apply_scaling(var=var) IN PLACE on the model of every event whose fit is ok (the others keep theirs).
        Returns the fits, one util.ScalingFit per event.  Sequence, ref_align and ref_like are not touched.  What this does to
        consensus accuracy on real data has not been measured."""
        _, stats = self.AlignStats(realign=True)
        return _recalibrate(self.events, stats, var, fit_kw)

    def KmerStats(self, groups=None, n_groups=None, realign=True):
        """Per event group and 5-mer state the sums of a re-estimation of that state's model rows (ps_kmer_stats): (scores, table).
        `groups` gives every event a group id 0 .. G - 1 — by default its strand, 0 template and 1 complement — and `n_groups` = G
        (1 .. 256; default 2 for strands, else the largest id + 1): the events of a group are taken to share what is wrong with
        their models.  realign=True aligns every event as ScoreEvents does (scores are its bits, float64 [E]) and reduces the
        alignment that leaves, on the device, in the same launch chain (k_kmer_stats); realign=False reduces ref_align as the
        events carry it, runs no DP and returns None for the scores.  table is a structured array (_capi.KMER_STATS [G, 1024]): n,
        sz, szz, sp, spu, spv for util.fit_kmers / util.fit_scaling_sd, every sum added serially — events in event order, levels
        ascending.  `self` is not modified.  ValueError for groups that do not fit."""
        grp, G = kmer_groups(self.events, groups, n_groups)
        with PSAlign._Data(self) as d:
            return _kmer_stats_on(d.api, d.h, self.events, grp, G, bool(realign))

    def RefitKmers(self, groups=None, n_groups=None, **fit_kw):
        """Re-estimate the models per k-mer on the alignment to self.sequence: one KmerStats() pass, util.fit_kmers(**fit_kw) per
        group, and util.apply_kmers IN PLACE on the model of every event of the group (a group without a fitted k-mer keeps its
        models).  Returns the fits, one util.KmerFit per group.  Sequence, ref_align and ref_like are not touched.  What this does
        to consensus accuracy on real data has not been measured."""
        grp, G = kmer_groups(self.events, groups, n_groups)
        _, table = self.KmerStats(grp, G, realign=True)
        fits = fit_kmers(table, **fit_kw)
        _refit_kmers(self.events, grp, fits)
        return fits

    def MoveStats(self, levels=False):
        """Per event the moves of its backtrace (ps_move_stats): (scores, records[, step, col]).  Every event is aligned as
        ScoreEvents does — scores are ScoreEvents' bits, as float64 [E] — and, on the device, between the backtrace walk and the
        kernel that overwrites its records, the moves of the path are counted (k_move_stats): records is a structured array
        (_capi.EVENT_MOVES [E]) with the cell the walk started from and stopped on, the recorded levels by move (match, ignore,
        insert, stay, extend) and the skips (runs, the longest, columns), for util.fit_transitions.  levels=True adds per event a
        uint8 array of move codes (_capi.MOVE_NAMES; 0: not on the path) and an int32 array of the columns the levels were
        recorded on — also for the inserted and ignored levels, where ref_align says -1.  Like ScoreEvents it does not write
        ref_align back; `self` is not modified.  A library without the entry point (the test-suite's checkers) walks its
        debug_fill tables: `util.moves_from_tables`."""
        with PSAlign._Data(self) as d:
            return _move_stats_on(d.api, d.h, self.events, self.params, bool(levels))

    def PosteriorStats(self, levels=False):
        """Per event the sum over ALL alignments in its band and the expected number of each move under it (ps_posterior_stats):
        records[, emit, col].  The lattice is the forward fill's on the refs the events carry; its recursion is the reference's
        with every maximum replaced by a log-sum (k_post_fwd), and a backward pass over the same cells weights every move by its
        posterior (k_post_bwd).  records is a structured array (_capi.EVENT_POSTERIOR [E]): logz — the marginal score, >= the
        event's ScoreEvents score —, e_skip .. e_extend for util.fit_transitions_soft, n_cells, n_cols, and inert = 1 with zeros for
        an event the reference would not fill.  levels=True adds per event two float64 arrays: the expected number of emitting
        arrivals at every level and their posterior mean column (NaN where there is none).  No backtrace runs; `self` is not
        modified.  A library without the entry point (the test-suite's checkers) runs the definition,
        `util.posterior_from_emissions`, on its debug_fill's band pattern."""
        with PSAlign._Data(self) as d:
            return _posterior_stats_on(d.api, d.h, self.events, self.params, bool(levels))

    def RefitTransitions(self, params=None, posterior=False, iters=1, **fit_kw):
        """Re-estimate the transition probabilities on the alignment to self.sequence: one MoveStats() pass, util.fit_transitions
        (**fit_kw) pooled per strand, starting from `params` ('skip_t' .. 'insert_c'; None: self.params; what it lacks is read off the events' models),
        and PSEvent.setparams IN PLACE on every event.  Returns the util.TransitionFit.  Sequence, ref_align, ref_like and the
        models' level tables are not touched.  What this does to consensus accuracy on real data has not been measured.
        posterior=True fits expected counts instead of the best path's: `iters` rounds of PosteriorStats() ->
        util.fit_transitions_soft(**fit_kw) -> setparams, every round starting from the rates the round before set (the bands do not
        move: a round is one call, no backtrace).  The fit returned is the last round's and gains `logz`, the list of the summed
        logz of all events before every round.  Equally unmeasured on real data."""
        base = self.params if params is None else params
        if not posterior:
            _, records = self.MoveStats()
            return _refit_transitions(self.events, records, strand_groups(self.events), base, fit_kw)
        return _refit_posterior(lambda: [self.PosteriorStats()], [self.events], base, iters, fit_kw)

    def ScoreSequences(self, seqs):
        """ndarray [len(seqs)][len(events)]: row s is what `pav = self.Copy(); pav.RealignTo(seqs[s]); pav.ScoreEvents()` returns,
        the loop of the reference's `variant -v` (Variant.py:52-59) — as ONE native call (ps_score_sequences: batched Smith-Waterman,
        the re-mapping of RealignTo on the device, all (sequence, event) alignments in one chain).  `self` is not modified.  Raises
        RealignTo's exception for a sequence whose identity is below its (sic) 0.6 %.  A library without the entry point (the
        test-suite's checkers) runs the literal loop, which is the definition of the result."""
        seqs = [str(s) for s in seqs]
        api = self._native()
        if "ps_score_sequences" in api.missing:
            rows = []
            for s in seqs:
                pav = self.Copy()
                pav.RealignTo(s)
                rows.append(pav.ScoreEvents())
            return np.array(rows, dtype=np.float64).reshape(len(seqs), len(self.events))
        with PSAlign._Data(self) as d:
            scores, acc = d.api.score_sequences(d.h, seqs, len(self.events))
        _check_realign_accuracy(acc)
        return scores

    def ScorePoints(self):
        """Score every single-base deletion / substitution / insertion (pyx:278-308)."""
        with PSAlign._Data(self, point_width=True) as d:
            hm = d.api.find_point_mutations(d.h)
            try:
                hs = d.api.score_mutations(d.h, hm)
            finally:
                d.api.muts_destroy(hm)
            try:
                return self._scores_to_py(d.api, hs)
            finally:
                d.api.muts_destroy(hs)

    def PointTable(self, table=True):
        """ScorePoints as arrays (ps_point_table): (table, margin, slot, n_positive) over the len(sequence) - 4 positions that
        FindPointMutations walks (the last four bases have no row), at `point_width` like ScorePoints.  table is float64 [n, 9] —
        slot 0 the deletion of the base, 1-4 its substitution by A / C / G / T (NaN for the base itself), 5-8 the insertion of
        A / C / G / T in front of it, each entry the score ScorePoints gives that edit — or None with table=False (it is then
        not copied back); margin [n] is the row's largest entry, slot [n] the first slot that holds it, n_positive [n] the
        entries > 0.  The reduction runs on the device (k_point_table); `self` is not modified.  A library without the entry
        point (the test-suite's checkers) builds the arrays from its scored list: `point_table_from_list`."""
        api = self._native()
        n = max(len(self.sequence) - 4, 0)
        with PSAlign._Data(self, point_width=True) as d:
            if "ps_point_table" in api.missing:
                hm = d.api.find_point_mutations(d.h)
                try:
                    hs = d.api.score_mutations(d.h, hm)
                finally:
                    d.api.muts_destroy(hm)
                try:
                    tb, margin, slot, npos = point_table_from_list(n, *d.api.muts_export(hs))
                finally:
                    d.api.muts_destroy(hs)
                return (tb if table else None), margin, slot, npos
            tb, best = d.api.point_table(d.h, n, want_table=table)
        return tb, best["margin"].copy(), best["slot"].copy(), best["n_positive"].copy()

    def ScoreMutations(self, muts):
        """Score the given MutationInfo list, same order (pyx:310-345)."""
        with PSAlign._Data(self) as d:
            hm = d.api.muts_create(muts)
            try:
                hs = d.api.score_mutations(d.h, hm)
            finally:
                d.api.muts_destroy(hm)
            try:
                return self._scores_to_py(d.api, hs)
            finally:
                d.api.muts_destroy(hs)

    def ScoreMutationSupport(self, muts=None, groups=None, n_groups=None):
        """Per-edit read support by event group (ps_score_mutation_support): (scores [M], support [M, G], scored list).
        `muts` is a MutationInfo list, scored as by ScoreMutations; None means every point edit (FindPointMutations' list) at
        `point_width`, as ScorePoints.  `groups` gives every event a group id 0 .. G - 1 — by default its strand, 0 template and
        1 complement (ev.model.complement) — and `n_groups` = G (1 .. 8; default 2 for strands, else the largest id + 1).
        scores are ScoreMutations' bit for bit and the scored list is what it returns.  support is a structured array
        (_capi.EDIT_SUPPORT): per edit and group `sum`, the group's events' terms added in event order (ALL its events: a read's
        term is not zero outside its aligned span), `cover`, the events of the group whose re-aligned span holds the edit
        (refstart <= start + 1 <= refend — a span test, not a likelihood test: a covering read's term can be zero), and `pos` /
        `neg`, the covering events with a positive / negative term.  The events x edits matrix stays on the device (k_support);
        `self` is not modified.  ValueError for groups that do not fit."""
        grp, G = support_groups(self.events, groups, n_groups)
        with PSAlign._Data(self, point_width=muts is None) as d:
            hm = d.api.find_point_mutations(d.h) if muts is None else d.api.muts_create(muts)
            try:
                return _support_on(d.api, d.h, hm, len(self.events), len(self.sequence), grp, G)
            finally:
                d.api.muts_destroy(hm)

    def ScoreMutationGenotypes(self, muts=None, alt_frac=(0.5,), groups=None, n_groups=None):
        """Genotype likelihoods per edit (ps_score_mutation_genotypes): (scores [M], support [M, G], scored list, lik [M, K + 1],
        n_cover [M]).  The first three are ScoreMutationSupport's, from the same call; `muts`, `groups` and `n_groups` as there.
        alt_frac gives K alt-allele fractions (0 .. 8, each 1e-6 .. 1 - 1e-6; util.alt_fractions(ploidy) for a ploidy):
        lik[:, k] is the sum over the events that SPAN the edit of log((1 - f_k) + f_k e^delta), the log-likelihood of a sample
        that carries the edit at fraction f_k relative to one that does not carry it (hom-ref, 0); lik[:, K] is hom-alt, the
        spanning events' terms added in event order; n_cover counts those events (the sum of support['cover'] over the groups).
        Only spanning events enter: a read's term is not zero outside its aligned span.  Reduced on the device (k_genotype), exp /
        log by the device library; `self` is not modified.  util.call_genotypes turns lik into GT / GQ / PL, uncalibrated.
        ValueError for groups or fractions that do not fit."""
        grp, G = support_groups(self.events, groups, n_groups)
        frac = check_alt_frac(alt_frac)
        with PSAlign._Data(self, point_width=muts is None) as d:
            hm = d.api.find_point_mutations(d.h) if muts is None else d.api.muts_create(muts)
            try:
                return _genotypes_on(d.api, d.h, hm, len(self.events), len(self.sequence), grp, G, frac)
            finally:
                d.api.muts_destroy(hm)

    def ScoreMutationPhase(self, muts, window=2, min_link=0.0, max_sets=4):
        """Phase of heterozygous edits (ps_score_mutation_phase): (scores [M], link [M, W], phase [M], hap [E, S], n_sets, scored
        list).  `muts` is the list of candidate sites — a driver passes its het calls sorted by position; any list is taken and
        "order" is list order — scored as by ScoreMutations (scores are its bits).  link[m, w - 1] (_capi.EDIT_LINK) compares, over
        the events that span both, "both alts on one chromosome copy" (cis) with "one alt on each" (trans) for the pair (m, m + w),
        w = 1 .. window (1 .. 8).  phase[m] (_capi.EDIT_PHASE) is a scan in list order: a site joins the set of the site before
        it when the vote of its links into that set is not 0 and at least min_link in size (hap -1 / +1: on the other / the same
        copy as the alt of the set's first site), else it opens a new set.  hap[e, k] (_capi.EVENT_HAP) adds event e's terms over
        the sites of set k (k < max_sets, 1 .. 8) by their hap: the event is from the first copy where lik1 > lik2.  All three
        are reduced on the device (k_link, k_phase, k_haptag) and return in one copy; `self` is not modified.  An edit's terms are
        treated as independent of the other edit of a pair, and everything here is uncalibrated.  util.call_phase turns phase
        into 0|1 / 1|0 and PS.  ValueError for arguments that do not fit."""
        W, lim, S = check_phase_args(window, min_link, max_sets)
        with PSAlign._Data(self) as d:
            hm = d.api.muts_create(muts)
            try:
                return _phase_on(d.api, d.h, hm, len(self.events), len(self.sequence), W, lim, S)
            finally:
                d.api.muts_destroy(hm)

    def ScoreMutationDeltas(self, muts):
        """ndarray [events][edits]: what each event adds to each edit's score (MakeMutations.cpp:51); `ScoreMutations` returns
        -1e-6 plus their sum in event order.  Not part of the reference's surface: the building block of event-sharded scoring
        (poreseq_amd.dist.score_mutations_event_sharded)."""
        with PSAlign._Data(self) as d:
            hm = d.api.muts_create(muts)
            try:
                return d.api.score_mutation_deltas(d.h, hm, len(self.events), len(muts))
            finally:
                d.api.muts_destroy(hm)

    def ApplyMuts(self, pymuts):
        """Greedy MakeMutations over already-scored mutations (pyx:347-375)."""
        with PSAlign._Data(self, point_width=True) as d:
            hm = d.api.muts_create(pymuts, with_scores=True)
            try:
                d.api.make_mutations(d.h, hm)
            finally:
                d.api.muts_destroy(hm)
            self.sequence = d.api.align_sequence(d.h)
            d.api.align_update_events(d.h, self.events)

    def Mutate(self, seqs='self', reps=4):
        """Seed-sequence driven consensus improvement (pyx:378-435).

        seqs: 'self' (every other event's own sequence), 'viterbi' (16 stochastic Viterbi
        seeds) or a list of strings.  Returns the total number of mutated bases.
        """
        with PSAlign._Data(self) as d:
            sequences = []
            if isinstance(seqs, str) and seqs == 'self':
                seqs = [x.sequence for x in self.events[::2]]
            elif isinstance(seqs, str) and seqs == 'viterbi':
                seqs = None
                sequences = d.api.viterbi_mutate(d.h, 16, 0.05, 0.01, 0.33, 0.75, self.params['verbose'])
            if seqs:
                sequences = list(seqs)
            totbases = 0
            for _ in range(reps):
                hm = d.api.find_mutations(d.h, sequences)
                try:
                    hs = d.api.score_mutations(d.h, hm)
                finally:
                    d.api.muts_destroy(hm)
                try:
                    nbases = d.api.make_mutations(d.h, hs)
                finally:
                    d.api.muts_destroy(hs)
                if nbases == 0:
                    break
                totbases += nbases
            self.sequence = d.api.align_sequence(d.h)
            d.api.align_update_events(d.h, self.events)
            return totbases

    def Refine(self):
        """Brute-force all single-base edits and apply the improving ones (pyx:437-472)."""
        with PSAlign._Data(self, point_width=True) as d:
            hm = d.api.find_point_mutations(d.h)
            try:
                hs = d.api.score_mutations(d.h, hm)
            finally:
                d.api.muts_destroy(hm)
            try:
                nbases = d.api.make_mutations(d.h, hs)
            finally:
                d.api.muts_destroy(hs)
            self.sequence = d.api.align_sequence(d.h)
            d.api.align_update_events(d.h, self.events)
            return nbases
