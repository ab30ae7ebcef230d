"""Lock-step refinement of several independent regions on one GPU.

The reference refines one region per process (cmdline.py:182-195); its regions are independent work-items.  One
region's calls keep a few percent of an MI355X busy, so the MI355X way to run many regions is not many processes or
threads but ONE host thread that issues every phase for all regions at once: `RegionBatch` mirrors the `PSAlign`
methods the consensus schedule uses (`Mutate`, `Refine`, `ScoreEvents`) over a list of `PSAlign` objects and drives
the `ps_batch_*` entry points of include/poreseq_hip.h, where each phase (Smith-Waterman batch, banded fills, edit
scoring, Viterbi) is one launch chain over all regions' events.

Results are those of running the same `PSAlign` calls region by region, bit for bit: every region owns a generator
(`ps_rng`, seeded like a fresh process) for ViterbiMutate's stochastic back-traces, and regions that have converged
simply drop out of the later rounds of a call, as their own `break` would.
"""
import numpy as np

from . import poreseqcpp


class RegionBatch:
    """A set of PSAlign objects (independent regions) refined in lock-step.  All methods work in place on the members."""

    def __init__(self, pas, api=None, resident=True):
        """resident=True keeps one native AlignData per region for the life of the batch: the events are marshalled and
        copied to the GPU once, every later call only announces itself (`ps_align_new_call` resets the scoring width and
        the seed-likelihood cache), and sequence / ref_align / ref_like are written back to the Python objects when the
        batch is closed (or by `sync()`).  The calls that only score (ScoreEvents, ScoreMutations, PointTable,
        ScoreMutationSupport) realign the events as a side effect, which the reference drops with its scratch AlignData
        (only ApplyMuts / Mutate / Refine write ref_align / ref_like back, pyx:375, 434, 471): the handle's refs are kept
        before such a call (`ps_align_keep_refs`) and put back after it, so the next call starts where a PSAlign would.
        resident=False rebuilds the AlignData for every call, as PythonToAlignData does (pyx:139-153); results are
        identical, whatever the order of the calls (tests/test_call_order.py)."""
        self.pas = list(pas)
        self.api = api if api is not None else (self.pas[0]._native() if self.pas else poreseqcpp._api())
        self.rngs = [self.api.rng_create(1) for _ in self.pas]   # rand() of a fresh process per region (Viterbi.cpp:108)
        self.resident = bool(resident)
        self._h = {}
        self._scratch = set()   # handles built for one scoring call by a library without ps_align_keep_refs (_open)

    def load(self, idx=None):
        """Create the resident AlignData of the regions `idx` now (e.g. before a timed section)."""
        for i in (range(len(self.pas)) if idx is None else idx):
            if self.resident and i not in self._h:
                pa = self.pas[i]
                self._h[i] = self.api.align_create(pa.sequence, pa.events, pa.params)
        return self

    def sync(self, idx=None):
        """Write sequence / ref_align / ref_like of resident regions back to their PSAlign objects."""
        for i in (list(self._h) if idx is None else idx):
            h = self._h.get(i)
            if h is not None:
                pa = self.pas[i]
                pa.sequence = self.api.align_sequence(h)
                self.api.align_update_events(h, pa.events)

    def drop(self, idx=None):
        """Forget the resident AlignData of the regions `idx` (default: all) WITHOUT writing anything back: the PSAlign objects
        were changed from outside (a new start sequence) and the next call rebuilds the AlignData from them."""
        for i in (list(self._h) if idx is None else idx):
            h = self._h.pop(i, None)
            if h is not None:
                self.api.align_destroy(h)

    def close(self):
        self.sync()
        for h in self._h.values():
            self.api.align_destroy(h)
        self._h = {}
        for r in self.rngs:
            self.api.rng_destroy(r)
        self.rngs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- plumbing ---------------------------------------------------------------------------------------------
    def _width(self, pa, point_width):
        return pa.params['point_width'] if (point_width and 'point_width' in pa.params) else pa.params.get('scoring_width', 150)

    def _open(self, idx, point_width=False, keep=False):
        """Native AlignData for the regions `idx`, as PythonToAlignData builds one per PSAlign call (pyx:139-153).  keep: the call
        only scores; a resident handle's refs are to come out of it as they went in (`_close` with write_back=False).  A library
        without ps_align_keep_refs (an older build of the test-suite's checkers) gets a scratch AlignData for such a call, built
        from the resident one's written-back state, as the reference does."""
        hs = []
        scratch = keep and self.resident and "ps_align_keep_refs" in self.api.missing
        for i in idx:
            pa = self.pas[i]
            if scratch:
                self.sync([i])
                h = self.api.align_create(pa.sequence, pa.events, pa.params)
                self.api.check(self.api.lib.ps_align_set_scoring_width(h, int(self._width(pa, point_width))))
                self._scratch.add(h.value)
            elif self.resident:
                self.load([i])
                h = self._h[i]
                self.api.check(self.api.lib.ps_align_new_call(h, int(self._width(pa, point_width))))
                if keep:
                    self.api.check(self.api.lib.ps_align_keep_refs(h))
            else:
                h = self.api.align_create(pa.sequence, pa.events, pa.params)
                if point_width and 'point_width' in pa.params:
                    self.api.check(self.api.lib.ps_align_set_scoring_width(h, int(pa.params['point_width'])))
            hs.append(h)
        return hs

    def _close(self, idx, hs, write_back=True):
        for i, h in zip(idx, hs):
            if h.value in self._scratch:
                self._scratch.discard(h.value)
                self.api.align_destroy(h)
                continue
            if self.resident:
                if write_back:
                    self.pas[i].sequence = self.api.align_sequence(h)   # cheap; refs follow at sync() / close()
                else:   # the end of a call that does not write back: kept refs return now, so that sync() reads them
                    self.api.check(self.api.lib.ps_align_new_call(h, int(self._width(self.pas[i], False))))
                continue
            if write_back:
                pa = self.pas[i]
                pa.sequence = self.api.align_sequence(h)
                self.api.align_update_events(h, pa.events)
            self.api.align_destroy(h)

    def _rounds(self, idx, hs, propose, reps):
        """reps x {propose -> ScoreMutations -> MakeMutations}; a region leaves when a round changes nothing (pyx:417-431)."""
        tot = {i: 0 for i in idx}
        live = list(range(len(idx)))
        for _ in range(reps):
            if not live:
                break
            lh = [hs[k] for k in live]
            hm = propose(live, lh)
            try:
                scored = self.api.batch_score_mutations(lh, hm)
            finally:
                for m in hm:
                    self.api.muts_destroy(m)
            try:
                nb = self.api.batch_make_mutations(lh, scored)
            finally:
                for m in scored:
                    self.api.muts_destroy(m)
            nxt = []
            for k, n in zip(live, nb):
                if n == 0:
                    continue
                tot[idx[k]] += n
                nxt.append(k)
            live = nxt
        return tot

    # -- the PSAlign calls of the consensus schedule, for the regions `idx` (default: all) ---------------------------
    def ScoreEvents(self, idx=None):
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        hs = self._open(idx, keep=True)
        try:
            sc = self.api.batch_score_alignments(hs, [len(self.pas[i].events) for i in idx])
        finally:
            self._close(idx, hs, write_back=False)
        return [s.tolist() for s in sc]

    def AlignStats(self, idx=None, realign=True):
        """PSAlign.AlignStats for the regions `idx` in lock-step: ONE ps_batch_align_stats call — with realign the launch chain of
        ScoreEvents over all regions, then one k_align_stats launch over all their events, one copy back.  Returns one (scores
        float64 [E] or None, stats _capi.EVENT_STATS [E]) per region; sequences and events are not modified (a resident handle's
        refs come out as they went in)."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        hs = self._open(idx, keep=True)
        try:
            if "ps_batch_align_stats" in self.api.missing:
                return [poreseqcpp._align_stats_on(self.api, h, self.pas[i].events, bool(realign)) for i, h in zip(idx, hs)]
            return self.api.batch_align_stats(hs, [len(self.pas[i].events) for i in idx], bool(realign))
        finally:
            self._close(idx, hs, write_back=False)

    def Recalibrate(self, idx=None, var=True, **fit_kw):
        """PSAlign.Recalibrate for the regions `idx`: one lock-step AlignStats, then util.fit_scaling / util.apply_scaling on the
        Python events' models.  A resident AlignData holds the models it was created with, so the handles of the regions whose
        models changed are written back (sync) and dropped; the next call rebuilds them.  Returns one list of fits per region."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        out = []
        for i, (_, stats) in zip(idx, self.AlignStats(idx, realign=True)):
            fits = poreseqcpp._recalibrate(self.pas[i].events, stats, var, fit_kw)
            if any(f.ok for f in fits) and i in self._h:
                self.sync([i])
                self.drop([i])
            out.append(fits)
        return out

    def _kmer_groups(self, idx, groups, n_groups):
        from .util import kmer_groups
        gs = [None] * len(idx) if groups is None else list(groups)
        ns = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * len(idx)
        if len(gs) != len(idx) or len(ns) != len(idx):
            raise ValueError("one grouping per region")
        return [kmer_groups(self.pas[i].events, g, n) for i, g, n in zip(idx, gs, ns)]

    def KmerStats(self, idx=None, groups=None, n_groups=None, realign=True):
        """PSAlign.KmerStats for the regions `idx` in lock-step: ONE ps_batch_kmer_stats call — with realign the launch chain of
        ScoreEvents over all regions, then one k_kmer_stats launch over all their events, one copy back.  `groups`: None (every
        region by strand) or one list of ids (or None) per region; `n_groups`: None, one number for all regions or one per region.
        Returns one (scores float64 [E] or None, table _capi.KMER_STATS [G, 1024]) per region; sequences and events are not
        modified (a resident handle's refs come out as they went in)."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        gg = self._kmer_groups(idx, groups, n_groups)
        hs = self._open(idx, keep=True)
        try:
            if "ps_batch_kmer_stats" in self.api.missing:
                return [poreseqcpp._kmer_stats_on(self.api, h, self.pas[i].events, g, G, bool(realign)) for i, h, (g, G) in zip(idx, hs, gg)]
            return self.api.batch_kmer_stats(hs, [len(self.pas[i].events) for i in idx], [g for g, _ in gg], [G for _, G in gg], bool(realign))
        finally:
            self._close(idx, hs, write_back=False)

    def RefitKmers(self, idx=None, pool=True, groups=None, n_groups=None, **fit_kw):
        """PSAlign.RefitKmers for the regions `idx`: one lock-step KmerStats, then util.fit_kmers / util.apply_kmers on the Python
        events' models.  pool=True (the regions carry the same reads' models under the same grouping) adds the regions' tables
        (util.add_kmer_stats, in the order of `idx`) and fits once for all of them; pool=False fits every region on its own table.
        A resident AlignData holds the models it was created with, so the handles of the regions whose models changed are written
        back (sync) and dropped; the next call rebuilds them.  Returns the fits per region, one util.KmerFit per group (with
        pool=True every region gets the same list)."""
        from .util import add_kmer_stats, fit_kmers
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        gg = self._kmer_groups(idx, groups, n_groups)
        tables = [t for _, t in self.KmerStats(idx, [g for g, _ in gg], [G for _, G in gg], realign=True)]
        if pool:
            if len(set(G for _, G in gg)) != 1:
                raise ValueError("RefitKmers(pool=True): the regions have different numbers of groups")
            fits = [fit_kmers(add_kmer_stats(tables), **fit_kw)] * len(idx)
        else:
            fits = [fit_kmers(t, **fit_kw) for t in tables]
        for i, (g, _), f in zip(idx, gg, fits):
            if poreseqcpp._refit_kmers(self.pas[i].events, g, f) and i in self._h:
                self.sync([i])
                self.drop([i])
        return fits

    def MoveStats(self, idx=None, levels=False):
        """PSAlign.MoveStats for the regions `idx` in lock-step: ONE ps_batch_move_stats call — the launch chain of ScoreEvents over
        all regions with one k_move_stats launch over all their events inside it, one copy back.  Returns one (scores float64 [E],
        records _capi.EVENT_MOVES [E][, step, col]) per region; sequences and events are not modified (a resident handle's refs
        come out as they went in)."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        hs = self._open(idx, keep=True)
        try:
            if "ps_batch_move_stats" in self.api.missing:
                return [poreseqcpp._move_stats_on(self.api, h, self.pas[i].events, self.pas[i].params, bool(levels))
                        for i, h in zip(idx, hs)]
            return self.api.batch_move_stats(hs, [[len(ev.mean) for ev in self.pas[i].events] for i in idx], bool(levels))
        finally:
            self._close(idx, hs, write_back=False)

    def PosteriorStats(self, idx=None, levels=False):
        """PSAlign.PosteriorStats for the regions `idx` in lock-step: ONE ps_batch_posterior_stats call — the band stage of the fills,
        k_post_fwd and k_post_bwd over all regions' events, one copy back.  Returns one records array (_capi.EVENT_POSTERIOR [E]) per
        region, with levels=True one (records, emit, col); no backtrace runs, and sequences, events and a resident handle's refs
        are not modified."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        hs = self._open(idx)
        try:
            if "ps_batch_posterior_stats" in self.api.missing:
                return [poreseqcpp._posterior_stats_on(self.api, h, self.pas[i].events, self.pas[i].params, bool(levels))
                        for i, h in zip(idx, hs)]
            return self.api.batch_posterior_stats(hs, [[len(ev.mean) for ev in self.pas[i].events] for i in idx], bool(levels))
        finally:
            self._close(idx, hs, write_back=False)

    def _refit_posterior(self, idx, pool, params, iters, fit_kw):
        """RefitTransitions(posterior=True): every round is one lock-step PosteriorStats; the handles are dropped after every round,
        since a resident AlignData holds the transition probabilities it was created with"""
        def stats(ids):
            def run():
                out = self.PosteriorStats(ids)
                for i in ids:
                    if i in self._h:
                        self.sync([i])
                        self.drop([i])
                return out
            return run
        if pool:
            fit = poreseqcpp._refit_posterior(stats(idx), [self.pas[i].events for i in idx],
                                              self.pas[idx[0]].params if params is None else params, iters, fit_kw)
            return [fit] * len(idx)
        return [poreseqcpp._refit_posterior(stats([i]), [self.pas[i].events], self.pas[i].params if params is None else params, iters, fit_kw)
                for i in idx]

    def RefitTransitions(self, idx=None, pool=True, params=None, posterior=False, iters=1, **fit_kw):
        """PSAlign.RefitTransitions for the regions `idx`: one lock-step MoveStats, then util.fit_transitions and PSEvent.setparams
        on the Python events.  pool=True (the regions carry reads of the same run) pools the records of all regions per strand and
        fits once for all of them; pool=False fits every region on its own records.  `params` as PSAlign.RefitTransitions takes
        it; None: every region's own pa.params (pool=True: those of the first region).  A resident AlignData holds the transition
        probabilities it was created with, so the handles of the regions are written back (sync) and dropped; the next call
        rebuilds them.  Returns one util.TransitionFit per region (with pool=True the same one).  posterior=True fits expected
        counts (PosteriorStats, util.fit_transitions_soft) in `iters` rounds, as PSAlign.RefitTransitions does: with pool=True every
        round is one lock-step call over all regions, with pool=False the regions are fitted one after the other."""
        from .util import strand_groups
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        if posterior:
            return self._refit_posterior(idx, pool, params, iters, fit_kw)
        recs = [r for _, r in self.MoveStats(idx)]
        grps = [strand_groups(self.pas[i].events) for i in idx]
        if pool:
            events = [ev for i in idx for ev in self.pas[i].events]
            fit = poreseqcpp._refit_transitions(events, np.concatenate(recs), [g for gs in grps for g in gs],
                                                 self.pas[idx[0]].params if params is None else params, fit_kw)
            fits = [fit] * len(idx)
        else:
            fits = [poreseqcpp._refit_transitions(self.pas[i].events, r, g, self.pas[i].params if params is None else params, fit_kw)
                    for i, r, g in zip(idx, recs, grps)]
        for i in idx:
            if i in self._h:
                self.sync([i])
                self.drop([i])
        return fits

    def ScoreSequences(self, seqs_per_region, idx=None):
        """PSAlign.ScoreSequences for the regions `idx` on their resident AlignData, all regions' sequences in one chain:
        seqs_per_region[k] are the candidate sequences of region idx[k] (may be empty).  Returns one ndarray
        [sequences][events] per region; nothing is modified."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        seqs = [[str(s) for s in sv] for sv in seqs_per_region]
        if len(seqs) != len(idx):
            raise ValueError("one list of sequences per region")
        if not idx:
            return []
        if "ps_batch_score_sequences" in self.api.missing:
            return [self.pas[i].ScoreSequences(sv) for i, sv in zip(idx, seqs)]
        hs = self._open(idx)
        try:
            res = self.api.batch_score_sequences(hs, seqs, [len(self.pas[i].events) for i in idx])
        finally:
            self._close(idx, hs, write_back=False)
        for _, acc in res:
            poreseqcpp._check_realign_accuracy(acc)
        return [sc for sc, _ in res]

    def PointTable(self, idx=None, table=True):
        """PSAlign.PointTable for the regions `idx` on their resident AlignData: ONE ps_batch_point_table call — the dense scoring
        chain of Refine over all regions, reduced on the device, one copy back.  Returns one (table or None, margin, slot,
        n_positive) per region; sequences and events are not modified (a resident handle's refs come out as they went in)."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        if "ps_batch_point_table" in self.api.missing:
            return [self.pas[i].PointTable(table) for i in idx]
        hs = self._open(idx, point_width=True, keep=True)
        try:
            ns = [max(int(self.api.lib.ps_align_sequence_length(h)) - 4, 0) for h in hs]
            res = self.api.batch_point_table(hs, ns, want_table=table)
        finally:
            self._close(idx, hs, write_back=False)
        return [(tb, b["margin"].copy(), b["slot"].copy(), b["n_positive"].copy()) for tb, b in res]

    def _lists(self, muts_per_region, idx):
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        lists = [None] * len(idx) if muts_per_region is None else [None if m is None else list(m) for m in muts_per_region]
        if len(lists) != len(idx):
            raise ValueError("one list of edits per region")
        return idx, lists

    def ScoreMutations(self, muts_per_region, idx=None):
        """PSAlign.ScoreMutations (`poreseq variant -m`) for the regions `idx` in lock-step: muts_per_region[k] is the MutationInfo
        list of region idx[k] (may be empty), all regions' lists scored by ONE ps_batch_score_mutations call.  Returns one
        MutationScore list per region, same order; sequences and events are not modified (a resident handle's refs come out as
        they went in)."""
        idx, lists = self._lists(muts_per_region, idx)
        if not idx:
            return []
        if any(m is None for m in lists):
            raise ValueError("one list of edits per region")
        hs = self._open(idx, keep=True)
        hm, scored = [], []
        try:
            hm = [self.api.muts_create(m) for m in lists]
            scored = self.api.batch_score_mutations(hs, hm)
            return [poreseqcpp._scored_list(*self.api.muts_export(s)) for s in scored]
        finally:
            for m in hm + scored:
                self.api.muts_destroy(m)
            self._close(idx, hs, write_back=False)

    def ScorePoints(self, idx=None):
        """PSAlign.ScorePoints for the regions `idx` in lock-step: every region's point edits at its `point_width`, scored by ONE
        ps_batch_score_mutations call.  Returns one MutationScore list per region; sequences and events are not modified."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return []
        hs = self._open(idx, point_width=True, keep=True)
        hm, scored = [], []
        try:
            hm = [self.api.find_point_mutations(h) for h in hs]
            scored = self.api.batch_score_mutations(hs, hm)
            return [poreseqcpp._scored_list(*self.api.muts_export(s)) for s in scored]
        finally:
            for m in hm + scored:
                self.api.muts_destroy(m)
            self._close(idx, hs, write_back=False)

    def _support(self, muts_per_region, idx, groups, n_groups, alt_frac=None):
        """ScoreMutationSupport (alt_frac None) and ScoreMutationGenotypes (one tuple of alt fractions for all regions, or a list of
        one per region) share everything but the native call: lists, groups, open / close and the path of a checker library"""
        points = muts_per_region is None
        idx, lists = self._lists(muts_per_region, idx)
        if not idx:
            return []
        if not points and any(m is None for m in lists):
            raise ValueError("one list of edits per region")
        groups = [None] * len(idx) if groups is None else list(groups)
        n_groups = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * len(idx)
        if len(groups) != len(idx) or len(n_groups) != len(idx):
            raise ValueError("one list of group ids per region")
        geno = alt_frac is not None
        fracs = [None] * len(idx)
        if geno:
            alt_frac = list(alt_frac)
            per_region = bool(alt_frac) and all(isinstance(f, (list, tuple, np.ndarray)) and np.ndim(f) == 1 for f in alt_frac)
            fracs = alt_frac if per_region else [alt_frac] * len(idx)
            if len(fracs) != len(idx):
                raise ValueError("one tuple of alt fractions for all regions or one per region")
            fracs = [poreseqcpp.check_alt_frac(f) for f in fracs]
        gG = [poreseqcpp.support_groups(self.pas[i].events, g, n) for i, g, n in zip(idx, groups, n_groups)]
        name = "ps_batch_score_mutation_genotypes" if geno else "ps_batch_score_mutation_support"
        hs = self._open(idx, point_width=points, keep=True)
        hm = []
        try:
            hm = [self.api.find_point_mutations(h) if points else self.api.muts_create(m) for h, m in zip(hs, lists)]
            if name in self.api.missing:
                if geno:
                    return [poreseqcpp._genotypes_on(self.api, h, m, len(self.pas[i].events), len(self.pas[i].sequence), g, G, f)
                            for i, h, m, (g, G), f in zip(idx, hs, hm, gG, fracs)]
                return [poreseqcpp._support_on(self.api, h, m, len(self.pas[i].events), len(self.pas[i].sequence), g, G)
                        for i, h, m, (g, G) in zip(idx, hs, hm, gG)]
            lists_x = [self.api.muts_export(m) for m in hm]
            n_muts, grps, Gs = [len(x[0]) for x in lists_x], [g for g, _ in gG], [G for _, G in gG]
            if geno:
                res = self.api.batch_score_mutation_genotypes(hs, hm, n_muts, grps, Gs, fracs)
                return [(sc, sup, poreseqcpp._scored_list(x[0], x[1], x[2], sc), lik, nc) for (sc, sup, lik, nc), x in zip(res, lists_x)]
            res = self.api.batch_score_mutation_support(hs, hm, n_muts, grps, Gs)
            return [(sc, sup, poreseqcpp._scored_list(x[0], x[1], x[2], sc)) for (sc, sup), x in zip(res, lists_x)]
        finally:
            for m in hm:
                self.api.muts_destroy(m)
            self._close(idx, hs, write_back=False)

    def ScoreMutationSupport(self, muts_per_region, idx=None, groups=None, n_groups=None):
        """PSAlign.ScoreMutationSupport for the regions `idx` in lock-step: ONE ps_batch_score_mutation_support call — one scoring
        chain over all regions, reduced per event group on the device, one copy back.  muts_per_region[k] is the MutationInfo list
        of region idx[k]; None instead of the lists means every region's point edits at `point_width`.  groups[k] / n_groups[k]
        (or one n_groups for all) as PSAlign.ScoreMutationSupport takes them, None for the strand default.  Returns one
        (scores, support, scored list) per region; sequences and the Python events are not modified."""
        return self._support(muts_per_region, idx, groups, n_groups)

    def ScoreMutationGenotypes(self, muts_per_region, idx=None, alt_frac=(0.5,), groups=None, n_groups=None):
        """PSAlign.ScoreMutationGenotypes for the regions `idx` in lock-step: ONE ps_batch_score_mutation_genotypes call — the
        scoring chain of ScoreMutationSupport over all regions, both reductions on the device, one copy back.  muts_per_region,
        groups and n_groups as ScoreMutationSupport takes them; alt_frac is one tuple of fractions for all regions or a list of
        one tuple (list, array) per region.  Returns one (scores, support, scored list, lik, n_cover) per region; sequences and
        the Python events are not modified."""
        return self._support(muts_per_region, idx, groups, n_groups, alt_frac=alt_frac)

    def ScoreMutationPhase(self, muts_per_region, idx=None, window=2, min_link=0.0, max_sets=4):
        """PSAlign.ScoreMutationPhase for the regions `idx` in lock-step: ONE ps_batch_score_mutation_phase call — one scoring chain
        over all regions, links, phase sets and read haplotypes reduced on the device, one copy back.  muts_per_region[k] is the
        list of candidate sites of region idx[k] (may be empty); window, min_link and max_sets are one value for all regions or a
        list of one per region.  Returns one (scores, link, phase, hap, n_sets, scored list) per region; sequences and the Python
        events are not modified."""
        idx, lists = self._lists(muts_per_region, idx)
        if not idx:
            return []
        if any(m is None for m in lists):
            raise ValueError("one list of edits per region")
        each = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * len(idx)
        args = list(zip(each(window), each(min_link), each(max_sets)))
        if len(args) != len(idx):
            raise ValueError("one window / min_link / max_sets for all regions or one per region")
        args = [poreseqcpp.check_phase_args(*a) for a in args]
        hs = self._open(idx, keep=True)
        hm = []
        try:
            hm = [self.api.muts_create(m) for m in lists]
            if "ps_batch_score_mutation_phase" in self.api.missing:
                return [poreseqcpp._phase_on(self.api, h, m, len(self.pas[i].events), len(self.pas[i].sequence), *a)
                        for i, h, m, a in zip(idx, hs, hm, args)]
            lists_x = [self.api.muts_export(m) for m in hm]
            res = self.api.batch_score_mutation_phase(hs, hm, [len(x[0]) for x in lists_x], [len(self.pas[i].events) for i in idx],
                                                      [a[0] for a in args], [a[1] for a in args], [a[2] for a in args])
            return [r + (poreseqcpp._scored_list(x[0], x[1], x[2], r[0]),) for r, x in zip(res, lists_x)]
        finally:
            for m in hm:
                self.api.muts_destroy(m)
            self._close(idx, hs, write_back=False)

    def Mutate(self, idx=None, seqs='self', reps=4):
        """PSAlign.Mutate (pyx:378-435) for the regions `idx`; returns {region index: total mutated bases}."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return {}
        hs = self._open(idx)
        try:
            if isinstance(seqs, str) and seqs == 'self':
                cand = [[x.sequence for x in self.pas[i].events[::2]] for i in idx]
            elif isinstance(seqs, str) and seqs == 'viterbi':
                cand = self.api.batch_viterbi_mutate(hs, [self.rngs[i] for i in idx], 16, 0.05, 0.01, 0.33, 0.75)
            else:
                cand = [list(seqs) for _ in idx]
            hseq = [self.api.seqs_create(c) for c in cand]
            try:
                tot = self._rounds(idx, hs, lambda live, lh: self.api.batch_find_mutations(lh, [hseq[k] for k in live]), reps)
            finally:
                for s in hseq:
                    self.api.seqs_destroy(s)
        except Exception:
            self._close(idx, hs, write_back=False)
            raise
        self._close(idx, hs)
        return tot

    def Refine(self, idx=None):
        """PSAlign.Refine (pyx:437-472) for the regions `idx`; returns {region index: mutated bases}."""
        idx = list(range(len(self.pas))) if idx is None else list(idx)
        if not idx:
            return {}
        hs = self._open(idx, point_width=True)
        try:
            tot = self._rounds(idx, hs, lambda live, lh: [self.api.find_point_mutations(h) for h in lh], 1)
        except Exception:
            self._close(idx, hs, write_back=False)
            raise
        self._close(idx, hs)
        return tot
