"""Host drivers that reproduce the *call schedule* of the reference's workflow layer on top of
`poreseqcpp.PSAlign`:

  consensus_region  <- poreseq/Mutate.py:8-101   (Mutate('self') then {Mutate('viterbi'), Refine()})
  test_start        <- poreseq/Mutate.py:59-65   (`test`: start from the read that spans the most of the draft)
  variant_region    <- poreseq/Variant.py:66-95  (ScoreMutations / ScorePoints with start offsetting)
  variant_points    <- poreseq/Variant.py:77-93  (`variant -a`: every point edit of one or many regions, as tables from one lock-step call)
  variant_sequences <- poreseq/Variant.py:48-63  (`variant -v`: whole candidate sequences, one batched ScoreSequences call)
  variant_support   <- poreseq/Variant.py:66-95  (`variant -m` over many regions in lock-step, with per-group read support; TSV or VCF)
  split_regions     <- poreseq/split_fasta.py:94-101 (max_length pieces with 1 kb overlap)

fast5 / BAM loading is out of scope: callers hand over a PSAlign whose events are already
loaded (synthetic here), exactly what `LoadAlignedEvents` would have returned.
"""
import sys

import numpy as np

from . import poreseqcpp
from .util import phred_from_margin


def _report(verbose, text):
    if verbose > 0:
        sys.stderr.write(text + "\n")


def test_start(events, refseq, summaries):
    """The start sequence of the reference's `test` mode (Mutate.py:59-65): one of the events' own base-called sequences
    instead of the draft.  `summaries[k]` is the Smith-Waterman summary of events[k].sequence against `refseq`
    (poreseqcpp.swalign_summaries).  Returns (sequence, index of the event it was cut from; -1 and "" when no event wins).

    The loop is the reference's, quirks included: an event's span on the DRAFT (last2 - first2) is compared with the LENGTH
    of the best slice so far and has to be strictly greater, so the first of equals stays; the 1-based first1 / last1 are used
    as 0-based slice bounds.  An empty alignment raises IndexError, as `pairs[-1]` of an empty list does there.
    """
    seq, chosen = "", -1
    for k, (ev, s) in enumerate(zip(events, summaries)):
        if s.n_pairs == 0:
            raise IndexError("list index out of range")
        if s.last2 - s.first2 > len(seq):
            seq, chosen = ev.sequence[s.first1:s.last1], k
    return seq, chosen


def _recalibrate_kw(recalibrate):
    """None / False: no recalibration; True: the defaults; a dict: keyword arguments of Recalibrate (var and util.fit_scaling's)"""
    if recalibrate is None or recalibrate is False:
        return None
    return dict(recalibrate) if isinstance(recalibrate, dict) else {}


def _refit_kmers_kw(refit_kmers):
    """None / False: no per-k-mer refit; True: the defaults; a dict: keyword arguments of RefitKmers (groups and util.fit_kmers')"""
    if refit_kmers is None or refit_kmers is False:
        return None
    return dict(refit_kmers) if isinstance(refit_kmers, dict) else {}


def _refit_transitions_kw(refit_transitions):
    """None / False: no transition refit; True: the defaults; a dict: keyword arguments of RefitTransitions (util.fit_transitions',
    and 'posterior': True / 'iters' for the fit of expected counts)"""
    if refit_transitions is None or refit_transitions is False:
        return None
    return dict(refit_transitions) if isinstance(refit_transitions, dict) else {}


def _rates_fitted(fit):
    return sum(1 for k in fit.rates if fit.flags.get(k) != 'empty')


def consensus_region(pa, params=None, reps=4, verbose=0, refseq=None, log=None, test=False, qualities=None, recalibrate=None, refit_kmers=False,
                     refit_transitions=False):
    """Run the consensus schedule in place on `pa`; returns (sequence, accuracy_vs_refseq).

    The call sequence is the reference's (Mutate.py:39-101) and has to be: a region with fewer than 5 events is handed
    back untouched (Mutate.py:50-53); otherwise Mutate('self', reps), then up to `reps` rounds of Mutate('viterbi')
    followed by Refine(), ending after the first Refine that changes nothing; `end_trim` bases come off both ends;
    the accuracy is the swalign identity against the sequence the region was loaded with.
    `log`, when given, receives (call, nbases, sequence) after every PSAlign call; `verbose` > 0 prints progress.
    `test` (Mutate.py:45-46, 59-68; `poreseq consensus -T`, and `poreseq train` unless --descend): the loaded sequence is thrown
    away and the schedule starts from `test_start`'s pick among the reads' own sequences, WITHOUT realignment — the events keep
    the ref_align they were loaded with; the accuracy is still taken against the loaded sequence.  It turns `verbose` 0 into 1.
    `qualities`, when given, is a list to which one entry is appended: the uint8 per-base qualities of the RETURNED sequence
    (util.phred_from_margin of one PointTable pass after the schedule's last call, cut by the same `end_trim` slice; uncalibrated),
    or None for a region handed back untouched.  The pass changes nothing else: sequence, accuracy, log and the events' ref_align /
    ref_like are what they are without it, and it draws no random numbers.
    `recalibrate` (not in the reference; off by default): True, or a dict of keyword arguments for it, runs one `pa.Recalibrate()`
    before Mutate('self') — every read's model shift / scale / var refitted on its alignment to the start sequence
    (util.fit_scaling), in place on the events' models — and logs ("Recalibrate", reads whose model changed, sequence).  None or
    False is the schedule as it is without the argument: same calls, same log, same random draws.  Unmeasured on real data.
    `refit_kmers` (not in the reference; off by default): True, or a dict of keyword arguments for it, runs one `pa.RefitKmers()`
    right after the optional recalibration and before Mutate('self') — per strand (or the given groups) and 5-mer state the level
    mean, level variance and stdv-channel mean re-estimated on the alignment to the start sequence (util.fit_kmers), in place on
    the events' models — and logs ("RefitKmers", k-mers fitted over the groups, sequence).  False or None is the schedule as it is
    without the argument.  What it does to accuracy on real data is unmeasured.
    `refit_transitions` (not in the reference; off by default): True, or a dict of keyword arguments for it, runs one
    `pa.RefitTransitions(params)` after the two refits above and before Mutate('self') — skip / stay / extend / insert per strand
    re-estimated from the moves of the backtrace on the start sequence (util.fit_transitions), set on the events through setparams
    — and logs ("RefitTransitions", rates fitted, sequence).  False or None is the schedule as it is without the argument.  What
    it does to accuracy on real data is unmeasured.
    """
    params = pa.params if params is None else params
    pa.params.setdefault('verbose', 0)
    identity = lambda a, b: poreseqcpp.swalign(a, b, pa._native)
    refseq = pa.sequence if refseq is None else refseq
    if test and verbose == 0:
        verbose = 1
    if len(pa.events) < 5:
        _report(verbose, "fewer than 5 events: region returned as loaded")
        if qualities is not None:
            qualities.append(None)
        return (refseq, 100)
    _report(verbose, "refining %d bases with %d events" % (len(refseq), len(pa.events)))
    if test:
        sums = poreseqcpp.swalign_summaries([(ev.sequence, refseq) for ev in pa.events], pa._native)
        pa.sequence, chosen = test_start(pa.events, refseq, sums)
        start = poreseqcpp.swalign_summaries([(pa.sequence, refseq)], pa._native)[0]
        _report(verbose, "starting from event %d: %d bases, identity %.1f%%" % (chosen, len(pa.sequence), start.accuracy))

    def call(name, fn):
        n = fn()
        if log is not None:
            log.append((name, n, pa.sequence))
        return n

    recal = _recalibrate_kw(recalibrate)
    if recal is not None:
        changed = call("Recalibrate", lambda: sum(1 for f in pa.Recalibrate(**recal) if f.ok))
        _report(verbose, "recalibrated the models of %d of %d reads" % (changed, len(pa.events)))
    refit = _refit_kmers_kw(refit_kmers)
    if refit is not None:
        fitted = call("RefitKmers", lambda: sum(f.n_fitted for f in pa.RefitKmers(**refit)))
        _report(verbose, "refitted %d k-mer rows" % fitted)
    retr = _refit_transitions_kw(refit_transitions)
    if retr is not None:
        fitted = call("RefitTransitions", lambda: _rates_fitted(pa.RefitTransitions(params=params, **retr)))
        _report(verbose, "refitted %d transition rates" % fitted)
    call("Mutate:self", lambda: pa.Mutate(reps=reps))
    if verbose > 0:
        _report(verbose, "identity after seeding from the reads: %.1f%%" % identity(pa.sequence, refseq)[0])
    for _ in range(reps):
        call("Mutate:viterbi", lambda: pa.Mutate(seqs='viterbi'))
        changed = call("Refine", pa.Refine)
        if verbose > 0:
            _report(verbose, "identity: %.1f%%" % identity(pa.sequence, refseq)[0])
        if changed == 0:
            break
    qual = None
    if qualities is not None:
        qual = phred_from_margin(pa.PointTable(table=False)[1], len(pa.sequence))
    trim = int(params['end_trim']) if 'end_trim' in params else 0
    if 'end_trim' in params and len(pa.sequence) > 2 * params['end_trim']:
        pa.sequence = pa.sequence[trim:-trim]
        if qual is not None:
            qual = qual[trim:-trim]
    if qualities is not None:
        qualities.append(qual)
    acc, pairs = identity(pa.sequence, refseq)
    if verbose > 0:
        gaps = np.sum(np.array(pairs) == 0, 0)
        _report(verbose, "final identity %.1f%%, %d insertions, %d deletions, coverage %.1fX"
                % (acc, gaps[0], gaps[1], np.mean(pa.Coverage())))
    return (pa.sequence, acc)


def consensus_regions(pas, params=None, reps=4, refseqs=None, logs=None, batch=None, resident=True, test=False, accuracies=None,
                      qualities=None, recalibrate=None, refit_kmers=False, refit_transitions=False):
    """The consensus schedule of `consensus_region` for several independent regions in lock-step (poreseq_amd.batch):
    every PSAlign call of the schedule is issued once for all regions that still take part in it, so each phase is one
    launch chain on the GPU.  Returns [(sequence, accuracy)] in the order of `pas`; each entry equals what
    `consensus_region(pa)` returns for that region run on its own from a fresh process.
    `logs`, when given, is a list of lists receiving (call, nbases, sequence) per region after every call.
    `batch`: an already loaded RegionBatch over `pas` (events resident on the GPU, see RegionBatch.load); it is closed here.
    `test`: every region starts from `test_start`'s pick instead of its loaded sequence (see consensus_region); the picks of all
    regions come from ONE batched Smith-Waterman call over all (read, draft) pairs.  Resident AlignData of a loaded `batch`
    still hold the loaded sequence: they are dropped and rebuilt from the PSAlign objects.
    `accuracies`, when given, is a list of lists receiving per region the identity against its refseq after Mutate('self') and
    after every Refine (the "Accuracy:" lines of Mutate.py:72-83), each round's values from one batched call over the live regions.
    The final accuracies likewise come from one batched call.
    `qualities`, when given, is a list that is set to one entry per region, in the order of `pas`: the uint8 per-base qualities of the
    returned sequence (see consensus_region), None for a region with fewer than 5 events.  They come from ONE lock-step
    RegionBatch.PointTable(table=False) over all refined regions after the schedule's last call; everything else the function returns
    or writes is bit for bit what it is without `qualities`.
    `recalibrate`: as consensus_region takes it; one lock-step RegionBatch.Recalibrate over all refined regions before Mutate('self'),
    logged per region as ("Recalibrate", reads whose model changed, sequence).  None or False: the schedule as it is without it.
    `refit_kmers`: as consensus_region takes it; one lock-step RegionBatch.RefitKmers(pool=False) over all refined regions — every
    region fitted on its own table, as consensus_region does — after the recalibration and before Mutate('self'), logged per region
    as ("RefitKmers", k-mers fitted over the groups, sequence).  Unmeasured on real data.
    `refit_transitions`: as consensus_region takes it; one lock-step RegionBatch.RefitTransitions(pool=False) over all refined regions
    — every region fitted on its own records, as consensus_region does — after the two refits above and before Mutate('self'),
    logged per region as ("RefitTransitions", rates fitted, sequence).  Unmeasured on real data.
    """
    from .batch import RegionBatch
    n = len(pas)
    refseqs = [pa.sequence for pa in pas] if refseqs is None else list(refseqs)
    out = [None] * n
    quals = [None] * n
    todo = []
    for i, pa in enumerate(pas):
        if 'verbose' not in pa.params:
            pa.params['verbose'] = 0
        if len(pa.events) < 5:                      # Mutate.py:50-53
            out[i] = (refseqs[i], 100)
        else:
            todo.append(i)
    if not todo and batch is not None:
        batch.close()                               # (every region had fewer than five events: nothing ran, the handles still go)
    if todo:
        api = pas[todo[0]]._native

        def note(i, call, nb):
            if logs is not None:
                logs[i].append((call, nb, pas[i].sequence))

        def identities(idx):
            if accuracies is not None and idx:
                sums = poreseqcpp.swalign_summaries([(pas[i].sequence, refseqs[i]) for i in idx], api)
                for i, s in zip(idx, sums):
                    accuracies[i].append(s.accuracy)

        if test:
            try:
                owner = [i for i in todo for _ in pas[i].events]
                sums = poreseqcpp.swalign_summaries([(ev.sequence, refseqs[i]) for i in todo for ev in pas[i].events], api)
                for i in todo:
                    pas[i].sequence = test_start(pas[i].events, refseqs[i], [s for o, s in zip(owner, sums) if o == i])[0]
                if batch is not None:
                    batch.drop(todo)
            except Exception:
                if batch is not None:
                    batch.drop()
                    batch.close()
                raise
        recal = _recalibrate_kw(recalibrate)
        refit = _refit_kmers_kw(refit_kmers)
        retr = _refit_transitions_kw(refit_transitions)
        with (batch if batch is not None else RegionBatch(pas, resident=resident)) as rb:
            if recal is not None:
                for i, fits in zip(todo, rb.Recalibrate(todo, **recal)):
                    note(i, "Recalibrate", sum(1 for f in fits if f.ok))
            if refit is not None:
                for i, fits in zip(todo, rb.RefitKmers(todo, pool=False, **refit)):
                    note(i, "RefitKmers", sum(f.n_fitted for f in fits))
            if retr is not None:
                for i, fit in zip(todo, rb.RefitTransitions(todo, pool=False, params=params, **retr)):
                    note(i, "RefitTransitions", _rates_fitted(fit))
            tot = rb.Mutate(todo, reps=reps)
            for i in todo:
                note(i, "Mutate:self", tot[i])
            identities(todo)
            live = list(todo)
            for _ in range(reps):
                if not live:
                    break
                tot = rb.Mutate(live, seqs='viterbi')
                for i in live:
                    note(i, "Mutate:viterbi", tot[i])
                nb = rb.Refine(live)
                for i in live:
                    note(i, "Refine", nb[i])
                identities(live)
                live = [i for i in live if nb[i] != 0]
            if qualities is not None:
                # the pass re-aligns the resident events like every ScoreMutations call: what the schedule left is written back
                # first, and the handles are forgotten afterwards, so that closing the batch writes nothing of it
                rb.sync(todo)
                for i, (_, margin, _, _) in zip(todo, rb.PointTable(todo, table=False)):
                    quals[i] = phred_from_margin(margin, len(pas[i].sequence))
                rb.drop(todo)
        for i in todo:
            pa = pas[i]
            p = pa.params if params is None else params
            if 'end_trim' in p and len(pa.sequence) > 2 * p['end_trim']:
                pa.sequence = pa.sequence[int(p['end_trim']):-int(p['end_trim'])]
                if quals[i] is not None:
                    quals[i] = quals[i][int(p['end_trim']):-int(p['end_trim'])]
        final = poreseqcpp.swalign_summaries([(pas[i].sequence, refseqs[i]) for i in todo], api)
        for i, s in zip(todo, final):
            out[i] = (pas[i].sequence, s.accuracy)
    if qualities is not None:
        qualities[:] = quals
    return out


def variant_region(pa, muts, region_start=0, params=None, out=None):
    """Score `muts` (or every point edit when the list is empty) as Variant.py:66-95 does: starts are
    region-relative inside the call and absolute again in the returned / printed MutationScores."""
    for m in muts:
        m.start -= region_start
    mutscores = pa.ScoreMutations(muts) if len(muts) > 0 else pa.ScorePoints()
    for ms in mutscores:
        ms.start += region_start
        if out is not None:
            out.write(str(ms) + '\n')
    return mutscores


def variant_points(pas, region_starts=None, params=None, out=None):
    """`poreseq variant -a` (Variant.py:77-93: every single-base deletion, substitution and insertion at every position) for one
    PSAlign or a list of them, all regions through ONE lock-step RegionBatch.PointTable call.  Returns (tables, percent): tables[r] =
    (table, margin, slot, n_positive) of region r as PSAlign.PointTable returns them, percent[r] the reference's '% positive
    variants' figure (Variant.py:80-93): the edits with a score > 0 among those with end_trim < start < len(sequence) - end_trim,
    in % (NaN when there are none).  With `out`, the lines that `variant_region(pa, [], region_starts[r], out=out)` writes are
    written region by region, in the reference's order — per position the deletion, the substitutions, the insertions, as
    str(MutationScore) with absolute starts — straight from the table.  No PSAlign is modified."""
    from .batch import RegionBatch
    single = isinstance(pas, poreseqcpp.PSAlign)
    pas = [pas] if single else list(pas)
    starts = [0] * len(pas) if region_starts is None else ([region_starts] if single else list(region_starts))
    if not pas:
        return [], []
    with RegionBatch(pas, resident=False) as rb:   # (not resident: nothing of the pass is written back to the PSAlign objects)
        tables = rb.PointTable(table=True)
    percent = []
    for pa, start0, (table, _margin, _slot, npos) in zip(pas, starts, tables):
        p = pa.params if params is None else params
        trim = p.get('end_trim', 0)
        pos = np.arange(table.shape[0])
        inside = (pos > trim) & (pos < len(pa.sequence) - trim)
        ntot = int(np.count_nonzero(~np.isnan(table[inside])))
        percent.append(100 * float(np.sum(npos[inside])) / ntot if ntot else float('nan'))
        if out is not None:
            dot = lambda c: c if len(c) else '.'
            lines = []
            for i, row in enumerate(table.tolist()):
                base, at = dot(pa.sequence[i]), i + start0
                lines.append('{}\t{}\t.\t{}\n'.format(at, base, row[0]))
                lines.extend('{}\t{}\t{}\t{}\n'.format(at, base, 'ACGT'[k], row[1 + k]) for k in range(4) if 'ACGT'[k] != pa.sequence[i])
                lines.extend('{}\t.\t{}\t{}\n'.format(at, 'ACGT'[k], row[5 + k]) for k in range(4))
            out.write(''.join(lines))
    return tables, percent


VCF_INFO = (("LLR", "1", "Float", "Log-likelihood change of the edit summed over all reads (natural log)"),
            ("DP", "1", "Integer", "Reads whose re-aligned span holds the edit (a span test, not a likelihood test)"),
            ("GDP", ".", "Integer", "Spanning reads per group"),
            ("GSUP", ".", "Integer", "Spanning reads per group that favour the edit (term > 0)"),
            ("GOPP", ".", "Integer", "Spanning reads per group that oppose the edit (term < 0)"),
            ("GLLR", ".", "Float", "Log-likelihood change per group, over all reads of the group"))
# (with a ploidy: the sample column.  GQ and PL are Phred-scaled ratios of this model's likelihoods: uncalibrated, like QUAL)
VCF_FORMAT = (("GT", "1", "String", "Genotype: the alt-copy count with the largest likelihood over the spanning reads (uncalibrated)"),
              ("GQ", "1", "Integer", "Genotype quality: the second smallest PL, at most 99 (uncalibrated)"),
              ("PL", "G", "Integer", "Phred-scaled genotype likelihoods over the spanning reads, 0 .. ploidy alt copies (uncalibrated)"))
# (with phase=True: the phase set of a phased het site)
VCF_FORMAT_PS = ("PS", "1", "Integer", "Phase set: POS of the first site of the set of phased het sites the record belongs to (uncalibrated)")


def vcf_fields(seq, start, orig, mut, offset=0):
    """(POS, REF, ALT) of the edit `start` (0-based in `seq`) orig -> mut; `offset` is added to POS (the region's start).  A
    replacement of equal length stands as it is (POS = start + 1); everything else is anchored on the base before it (POS =
    start), and at start 0, where there is none, on the base after `orig`, which is appended to both alleles (POS = 1)."""
    if len(orig) == len(mut) and len(orig) > 0:
        return start + 1 + offset, orig, mut
    if start > 0:
        a = seq[start - 1:start]
        return start + offset, a + orig, a + mut
    a = seq[len(orig):len(orig) + 1]
    return 1 + offset, orig + a, mut + a


def vcf_qual(score):
    """QUAL of a record: clip(floor(score * 10 / ln 10 + 0.5), 0, 9999), the Phred scale of the likelihood ratio.  UNCALIBRATED, as
    the FASTQ qualities are (util.phred_from_margin): a ratio of this model, not a measured error rate."""
    q = np.floor(float(score) * 10.0 / np.log(10.0) + 0.5)
    return int(min(max(q, 0.0), 9999.0)) if q == q else 0


def variant_support(pas, muts_per_region, region_starts=None, groups=None, group_names=("t", "c"), out=None, fmt="tsv", chrom="region",
                    min_score=0.0, ploidy=None, sample="sample", phase=False, min_gq=20, window=2, min_link=0.0):
    """`poreseq variant -m` for one PSAlign or a list of them with the read evidence behind every score: all regions go through ONE
    lock-step RegionBatch.ScoreMutationSupport call.  muts_per_region[r] is the MutationInfo list of region r with ABSOLUTE starts
    (region_starts[r] is subtracted inside the call and added again outside, as variant_region does — on copies: the lists handed
    in are not changed); None means every point edit of every region.  groups[r] gives every event of region r a group id below
    len(group_names); None is the strand default, template 0 / complement 1, which the default names ("t", "c") fit.
    Returns one (scores, support, scored list) per region, as PSAlign.ScoreMutationSupport does, the scored starts absolute.
    fmt="tsv": one '#' header line (MutationInfo reads it as a comment), then per edit str(MutationScore) — the reference's four
      columns, byte for byte what variant_region writes — followed per group by tab-separated cover, pos, neg, sum.
    fmt="vcf": a VCF 4.2 header and one record per edit with score > min_score, in list order (`vcf_fields`, `vcf_qual`); `chrom`
      is one name or one per region.  INFO = LLR=<score>;DP=<sum of cover>;GDP=..;GSUP=..;GOPP=..;GLLR=.., the G-tags
      comma-separated per group in group order.
    ploidy=P (1 .. 9) adds a genotype per edit: the regions go through ONE RegionBatch.ScoreMutationGenotypes call with
      util.alt_fractions(P) instead, every returned tuple gains (lik, n_cover), and util.call_genotypes writes them out — the VCF
      gets FORMAT lines for GT, GQ and PL, the column `sample` and GT:GQ:PL per record (which records appear is unchanged); the TSV
      gets the columns n_cover, gt, gq and gl_0 .. gl_P, the natural-log likelihood of 0 .. P alt copies relative to hom-ref.
      ploidy=None is the output without them, byte for byte.
    phase=True (needs ploidy=2, ValueError otherwise) phases the het calls: per region the records that are written (VCF: score >
      min_score; TSV: all) with GT 0/1 and GQ >= min_gq, stably sorted by start, go through ONE lock-step
      RegionBatch.ScoreMutationPhase call (window, min_link; on AlignData of their own, as every call here).  util.call_phase
      turns a het site in a set of two or more into 0|1 / 1|0; the VCF gets a FORMAT line for PS and GT:GQ:PL:PS per record, PS the
      POS of the set's first site or '.'; the TSV gets the columns phase_set (the absolute start of the set's first site), hap and
      vote, '.' where there is none.  Every returned tuple gains (event haplotypes int8 [E]: 1 where lik1 > lik2 for phase set 0,
      2 where lik2 > lik1, else 0; the record (site indices into the list, link, phase, hap, n_sets) of the region's phase call).
      phase=False writes the same bytes and returns the same tuples as without it.
    `cover` is a span test, not a likelihood test, and QUAL, GQ and PL are uncalibrated.  No PSAlign is modified."""
    from .batch import RegionBatch
    from .util import MutationInfo, alt_fractions, call_genotypes, call_phase, check_phase_args
    if fmt not in ("tsv", "vcf"):
        raise ValueError("variant_support: fmt is 'tsv' or 'vcf'")
    if phase and ploidy != 2:
        raise ValueError("variant_support: phase=True needs ploidy=2")
    if phase:
        check_phase_args(window, min_link, 4)
    fracs = None if ploidy is None else alt_fractions(ploidy)
    single = isinstance(pas, poreseqcpp.PSAlign)
    pas = [pas] if single else list(pas)
    if single:
        muts_per_region = None if muts_per_region is None else [muts_per_region]
        groups = None if groups is None else [groups]
    starts = [0] * len(pas) if region_starts is None else ([region_starts] if single else list(region_starts))
    chroms = [chrom] * len(pas) if isinstance(chrom, str) else list(chrom)
    names = [str(n) for n in group_names]
    rel = None
    if muts_per_region is not None:
        rel = []
        for ml, s0 in zip(muts_per_region, starts):
            row = []
            for m in ml:
                mi = MutationInfo()
                mi.start, mi.orig, mi.mut = int(m.start) - int(s0), m.orig, m.mut
                row.append(mi)
            rel.append(row)
    res = []
    if pas:
        with RegionBatch(pas, resident=False) as rb:   # (not resident: nothing of the pass is written back to the PSAlign objects)
            if ploidy is None:
                res = rb.ScoreMutationSupport(rel, groups=groups, n_groups=len(names))
            else:
                res = rb.ScoreMutationGenotypes(rel, alt_frac=fracs, groups=groups, n_groups=len(names))
    called = [call_genotypes(one[3], one[4], ploidy) for one in res] if ploidy is not None else []
    pcols = [None] * len(pas)      # per region and edit what the phase adds: (GT, PS or None, vote, hap) for the sites of the phase call
    if phase and pas:
        picks = []
        for one, (gts, gqs, _pls), s0 in zip(res, called, starts):
            keep = [i for i, ms in enumerate(one[2]) if gts[i] == '0/1' and gqs[i] >= min_gq and (fmt == "tsv" or ms.score > min_score)]
            picks.append(sorted(keep, key=lambda i: one[2][i].start))     # (stable: equal starts keep their list order)
        sites = []
        for one, pick in zip(res, picks):
            row = []
            for i in pick:
                mi = MutationInfo()
                mi.start, mi.orig, mi.mut = one[2][i].start, one[2][i].orig, one[2][i].mut     # (still relative to the region)
                row.append(mi)
            sites.append(row)
        with RegionBatch(pas, resident=False) as rb:
            ph = rb.ScoreMutationPhase(sites, window=window, min_link=min_link, max_sets=4)
        out_res = []
        for r, (pa, one, pick, p, s0) in enumerate(zip(pas, res, picks, ph, starts)):
            _sc, plink, pphase, phap, nsets, _scored = p
            if fmt == "vcf":
                at = [vcf_fields(pa.sequence, one[2][i].start, one[2][i].orig, one[2][i].mut, int(s0))[0] for i in pick]
            else:
                at = [one[2][i].start + int(s0) for i in pick]
            pgt, pps = call_phase(['0/1'] * len(pick), pphase, at)
            pcols[r] = {i: (g, q, float(v), int(h)) for i, g, q, v, h in zip(pick, pgt, pps, pphase["vote"].tolist(), pphase["hap"].tolist())}
            tag = np.zeros(len(pa.events), dtype=np.int8)
            if phap is not None and phap.shape[0] and phap.shape[1]:
                tag[phap["lik1"][:, 0] > phap["lik2"][:, 0]] = 1
                tag[phap["lik2"][:, 0] > phap["lik1"][:, 0]] = 2
            out_res.append(tuple(one) + (tag, (pick, plink, pphase, phap, nsets)))
        res = out_res
    if out is not None:
        if fmt == "tsv":
            out.write('#start\torig\tmut\tscore' + ''.join('\tcover_{0}\tpos_{0}\tneg_{0}\tsum_{0}'.format(n) for n in names) +
                      ('' if ploidy is None else '\tn_cover\tgt\tgq' + ''.join('\tgl_{}'.format(k) for k in range(int(ploidy) + 1))) +
                      ('\tphase_set\thap\tvote' if phase else '') + '\n')
        else:
            out.write('##fileformat=VCFv4.2\n##source=poreseq_amd.variant_support\n')
            for tag, num, typ, desc in VCF_INFO:
                per = '' if num == '1' else ' (groups: {})'.format(','.join(names))
                out.write('##INFO=<ID={},Number={},Type={},Description="{}{}">\n'.format(tag, num, typ, desc, per))
            if ploidy is not None:
                for tag, num, typ, desc in VCF_FORMAT + ((VCF_FORMAT_PS,) if phase else ()):
                    out.write('##FORMAT=<ID={},Number={},Type={},Description="{}">\n'.format(tag, num, typ, desc))
            out.write('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO' + ('' if ploidy is None else '\tFORMAT\t{}'.format(sample)) + '\n')
    for r, (pa, s0, ch, one) in enumerate(zip(pas, starts, chroms, res)):
        scores, sup, scored = one[:3]
        lines = []
        gcol = [''] * len(scored)      # what a genotype adds behind every line
        if ploidy is not None:
            gts, gqs, pls = called[r]
            if phase:      # the phased GT where there is one
                gts = [pcols[r][i][0] if i in pcols[r] else gt for i, gt in enumerate(gts)]
            if fmt == "tsv":
                gcol = ['\t{}\t{}\t{}\t0.0'.format(nc, gt, gq) + ''.join('\t' + repr(v) for v in row)
                        for nc, gt, gq, row in zip(np.asarray(one[4]).tolist(), gts, gqs, np.asarray(one[3], dtype=np.float64).tolist())]
                if phase:
                    dot = lambda v: '.' if v is None else str(v)
                    gcol = [g + ('\t{}\t{}\t{}'.format(dot(pcols[r][i][1]), pcols[r][i][3], repr(pcols[r][i][2])) if i in pcols[r] else '\t.\t.\t.')
                            for i, g in enumerate(gcol)]
            elif phase:
                gcol = ['\tGT:GQ:PL:PS\t{}:{}:{}:{}'.format(gt, gq, ','.join(str(p) for p in pl),
                                                           pcols[r][i][1] if i in pcols[r] and pcols[r][i][1] is not None else '.')
                        for i, (gt, gq, pl) in enumerate(zip(gts, gqs, pls))]
            else:
                gcol = ['\tGT:GQ:PL\t{}:{}:{}'.format(gt, gq, ','.join(str(p) for p in pl)) for gt, gq, pl in zip(gts, gqs, pls)]
        for ms, rec, gc in zip(scored, sup.tolist(), gcol):
            if fmt == "tsv":
                ms.start += int(s0)
                lines.append(str(ms) + ''.join('\t{}\t{}\t{}\t{}'.format(r[1], r[2], r[3], r[0]) for r in rec) + gc + '\n')
                continue
            if ms.score > min_score:
                pos, ref, alt = vcf_fields(pa.sequence, ms.start, ms.orig, ms.mut, int(s0))
                col = lambda k: ','.join(str(r[k]) for r in rec)
                info = 'LLR={};DP={};GDP={};GSUP={};GOPP={};GLLR={}'.format(ms.score, sum(r[1] for r in rec), col(1), col(2), col(3), col(0))
                lines.append('{}\t{}\t.\t{}\t{}\t{}\t.\t{}{}\n'.format(ch, pos, ref, alt, vcf_qual(ms.score), info, gc))
            ms.start += int(s0)
        if out is not None:
            out.write(''.join(lines))
    return res[0] if single and res else res


def variant_sequences(pa, variants, out=None):
    """Score whole candidate sequences against the reads as `poreseq variant -v` does (Variant.py:48-63): `variants` is a mapping
    id -> sequence or an iterable of (id, sequence); returns {id: dscore}, dscore = sum of the events' scores after re-aligning a
    copy of `pa` to the sequence, minus the same sum for `pa` as it is, and writes the reference's 'id, dscore' line per variant to
    `out`.  All variants go through ONE `PSAlign.ScoreSequences` call; `pa` is not modified.  The sums are numpy's, on the host,
    so the additions happen in the reference's order."""
    items = list(variants.items()) if hasattr(variants, "items") else [(k, v) for k, v in variants]
    basescore = np.sum(pa.ScoreEvents())
    rows = pa.ScoreSequences([str(seq) for _, seq in items])
    variantscores = {}
    for (vid, _), row in zip(items, rows):
        dscore = np.sum(row) - basescore
        if out is not None:
            out.write('{}, {}\n'.format(vid, dscore))
        variantscores[vid] = dscore
    return variantscores


def train(make_pa, params, refseq, iters=1, reps=10, save=None, paramlists=None, in_flight=1, lock_step=False, test=False, estimate=False):
    """Transition-parameter search of `poreseq train` (cmdline.py:246-267): every iteration runs the consensus schedule
    (reps = 10) once per candidate parameter set (VaryParams: 16 of them) on the same region and keeps the most accurate.

    make_pa(params) returns a freshly loaded PSAlign of the training region whose event models carry the transition
    probabilities of `params` (LoadAlignedEvents + setparams in the reference).  `paramlists` (optional, one list per
    iteration) replaces VaryParams, e.g. for reproducible tests.  Returns (best params, best accuracy per iteration).

    The candidates are independent replicas of one region:
      lock_step=True   all of them go through the schedule as ONE lock-step batch (poreseq_amd.batch): a single launch
                       chain per phase, the GPU-native mode.  Each replica draws its stochastic Viterbi seeds from the
                       generator of a fresh process, i.e. the result is that of 16 separate `poreseq consensus` runs.
      in_flight=k      k replicas at a time on host threads (same random-stream semantics as lock_step).
      default          one after another in this thread: replica k continues the rand() stream where replica k-1
                       stopped, which is what the reference's single process does — bit-parity mode.
    Which candidate wins can differ between the first two and the last by the luck of the seeds; keep the default
    when comparing against the reference.

    `test` is handed to the consensus schedule of every candidate, in all three modes.  The reference's command line runs
    its candidates with test = not --descend (cmdline.py:242-244), i.e. `poreseq train` corresponds to test=True here and
    `poreseq train --descend` to the default, test=False.

    `estimate` (not in the reference; off by default): the search starts from the transition probabilities fitted to the moves of
    one forward pass — make_pa(params).RefitTransitions(params), util.fit_transitions — instead of the given ones; every other
    key of `params` stays.  estimate='posterior' fits the EXPECTED moves under the sum over all alignments in the bands instead
    (RefitTransitions(posterior=True), util.fit_transitions_soft).  Both unmeasured on real data.
    """
    from .util import VaryParams, SaveParams
    if estimate:
        fit = make_pa(params).RefitTransitions(params=params, posterior=estimate == 'posterior')
        params = dict(params)
        params.update({k: fit.params[k] for k in fit.rates})
    best_accs = []
    for it in range(iters):
        cands = paramlists[it] if paramlists is not None else VaryParams(params)

        def one(p):
            return consensus_region(make_pa(p), p, reps=reps, refseq=refseq, test=test)[1]

        if lock_step:
            pas = [make_pa(p) for p in cands]
            accs = [acc for _, acc in consensus_regions(pas, None, reps=reps, refseqs=[refseq] * len(pas), test=test)]
        elif in_flight > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=int(in_flight)) as pool:
                accs = list(pool.map(one, cands))
        else:
            accs = [one(p) for p in cands]
        params = cands[int(np.argmax(accs))]
        if save:
            SaveParams(save, params)
        best_accs.append(max(accs))
    return params, best_accs


def split_regions(length, region_length=10000):
    """[(start, end)] region work-items: region_length pieces stepping by region_length - 1000
    (split_fasta.py:94-101; a 35 000-base sequence gives 0:10000, 9000:19000, 18000:28000, 27000:35000)."""
    region_length = int(region_length)
    out = []
    dl = region_length - 1000
    istart, iend = 0, min(region_length, length)
    while istart < iend:
        out.append((istart, iend))
        iend = min(iend + dl, length)
        istart = min(istart + dl, length)
    return out


def merge_seqs(seq1, seq2, overlap=1000, swalign=None):
    """Stitch two region sequences whose ends share about `overlap` bases: the tail of `seq1` is aligned with the head
    of `seq2` and the join is made at the middle aligned pair.

    Index arithmetic as merge_fasta.py:8-39, quirks included, so that stitched assemblies are identical: a `seq2` shorter
    than the overlap contributes all but its last base to the alignment; the identity threshold compares a percentage
    with 0.70; the cut into `seq1` is counted from its END (a middle pair on the tail's last base therefore cuts at 0,
    i.e. drops `seq1` — the reference's behaviour for degenerate overlaps).
    """
    swalign = poreseqcpp.swalign if swalign is None else swalign
    tail_from = -overlap if len(seq1) >= overlap else 0
    head_to = overlap if len(seq2) >= overlap else len(seq2) - 1
    acc, pairs = swalign(seq1[tail_from:], seq2[:head_to])
    if acc < 0.70:
        raise Exception('Insufficient accuracy for overlap')
    both = [(a, b) for a, b in pairs if a > 0 and b > 0]
    a_mid, b_mid = both[int(len(both) / 2)]
    return seq1[:tail_from + a_mid] + seq2[b_mid:]


def polish(sequence, make_region_pa, params=None, region_length=10000, overlap=1000, batch=16, reps=4, refine=None, swalign=None):
    """Assembly polish = the reference's split -> consensus per region -> merge pipeline (split_fasta.py:50-133,
    `poreseq consensus` per region file, merge_fasta.py:41-80) as one call.

    sequence         the draft to polish (only its length and the region coordinates are used here)
    make_region_pa   callable (start, end) -> PSAlign loaded with the draft slice and the events overlapping it
                     (what LoadAlignedEvents returns for region 'start:end')
    batch            regions refined in lock-step per GPU (poreseq_amd.batch); `refine` replaces the default
                     `poreseq_amd.dist.refine_regions` (regions sharded over the ranks of the process group, longest first)
    swalign          the Smith-Waterman the stitching uses (default: this package's, on the GPU; tests of the driver pass a checker's)
    Returns (polished sequence, [(start, end, region consensus, accuracy)]).  With an `end_trim` in `params` the region
    sequences lose that many bases per end before stitching, exactly as the region FASTA files of the reference do.
    """
    from . import dist as psdist
    regs = split_regions(len(sequence), region_length)
    refine = psdist.refine_regions if refine is None else refine
    done = refine(regs, make_region_pa, params=params, batch=batch, reps=reps)
    merged = done[0][0]
    for seq, _ in done[1:]:
        merged = merge_seqs(merged, seq, overlap, swalign)
    return merged, [(a, b, s, acc) for (a, b), (s, acc) in zip(regs, done)]
