/*
 * poreseq_hip.h — C ABI of libporeseq_hip.so, the MI355X (gfx950) implementation of
 * PoreSeq's event-level HMM scoring path.
 *
 * Every entry point replaces one function the reference's Cython binding
 * (poreseq/_poreseqcpp.pyx) calls in the reference C++ core; the reference
 * interface each one stands in for is cited as file:line relative to the
 * reference tree.  Only plain pointers and sizes cross this boundary.
 * A few entry points go beyond the reference's surface and reduce its scores on the device: ps_point_table (a row per position)
 * and ps_score_mutation_support (per edit and event group: the summed terms, the reads that span the edit and how many of
 * them favour or oppose it) with ps_score_mutation_genotypes (per edit: the likelihood of every alt-allele fraction asked for,
 * over the reads that span the edit) and ps_score_mutation_phase (pair links between candidate sites, phase sets and a haplotype per read).
 * `cover` there is a span test on the re-aligned reads, not a likelihood test, and anything
 * Phred-scaled that drivers derive from these scores is uncalibrated.
 *
 * All functions return PS_OK (0) or a negative ps_status; ps_last_error()
 * gives the message of the last failure on the calling thread.  The library
 * never falls back to a CPU implementation: without a usable HIP device every
 * compute call fails with PS_ERR_NO_DEVICE.
 *
 * Threading: every host thread that calls into the library gets its own runtime (HIP streams and device
 * buffer pools), so independent ps_align handles may be driven concurrently from different threads — the
 * way to keep an MI355X busy with many independent regions.  One handle must not be shared between
 * threads.  The uniform deviates of ps_viterbi_mutate come from a per-thread generator (see ps_srand).
 *
 * Indices follow the reference: mutation `start` is a 0-based base index,
 * ref_align values are 1-based state indices (0 = unaligned, -1 = inserted
 * level), Smith-Waterman index lists are 1-based with 0 = gap.
 *
 * Domain of ref_align: any double.  A level is aligned iff its entry is > 0 (an entry in (0, 1) is
 * column 0, a fraction truncates; NaN, 0 and -1 are not aligned).  ps_align_create, ps_align_stats and
 * the scoring calls take every value.  ViterbiMutate walks the positions from (int)ref_align of the
 * first aligned level to that of the last: an entry that is not below 2^31 (+inf included) has no
 * defined conversion, and ps_viterbi_mutate, ps_batch_viterbi_mutate and ps_debug_viterbi answer
 * PS_ERR_BAD_ARG for it, naming the event and the level, before any kernel of the call.  The walk is
 * linear in the largest entry.
 */
#ifndef PORESEQ_HIP_H_
#define PORESEQ_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_N_STATES 1024 /* cpp/AlignUtil.h:19 */

typedef enum ps_status {
    PS_OK = 0,
    PS_ERR_BAD_ARG = -1,     /* NULL pointer, negative size, negative mutation start ... */
    PS_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at init */
    PS_ERR_HIP = -3,         /* a HIP call failed */
    PS_ERR_UNSUPPORTED = -4, /* e.g. a band footprint beyond 2046 rows on one anti-diagonal (realign_width > 1022 in the worst case) */
    PS_ERR_NOMEM = -5
} ps_status;

const char* ps_last_error(void);
/* Name of the backend that serves this ABI ("hip-gfx950"); the test-only
 * oracle and reference shims answer "oracle-cpu" / "reference-cpp". */
const char* ps_backend_name(void);
/* One line about the process-wide state of the library, for logs and bench lines: how its streams get hardware queues (every
 * stream on one priority level with a queue each — GPU_MAX_HW_QUEUES >= 8 was in force when HIP started — or dealt over the
 * device's priority levels), runtimes (host threads inside the library), the per-runtime memory share and the slabs that hold
 * full score matrices.  A host that binds the C ABI directly and wants the first mode starts its process with GPU_MAX_HW_QUEUES=12
 * (or more) in the environment.  Launches nothing (it may start the HIP runtime to ask the device for its memory size). */
int ps_info(char* out, int64_t cap);

/* AlignParams — cpp/AlignUtil.h:57-66 (defaults 4.5 / 150 / 300 / 0). */
typedef struct ps_params {
    double lik_offset;
    int32_t scoring_width;
    int32_t realign_width;
    int32_t verbose;
} ps_params;

/* ---- AlignData (cpp/AlignData.h:26-35): sequence + events + params (+ seed-likelihood cache) ---- */
typedef struct ps_align ps_align;

/* Replaces PythonToAlignData / PythonToEvents (_poreseqcpp.pyx:99-153), i.e.
 * Sequence(seq) (cpp/Sequence.h:31-34), EventData::setData (cpp/EventData.h:208-224),
 * ModelData::setData / setParams (cpp/EventData.h:48-73).
 *   level_off[E+1]      CSR offsets of each event's levels in mean/stdv/ref_align/ref_like
 *   model[E][4][1024]   level_mean, level_stdv, sd_mean, sd_stdv
 *   trans[E][4]         prob_skip, prob_stay, prob_extend, prob_insert
 *   evseq/evseq_off     each event's own 2D base-called sequence (may be NULL)
 * Everything is copied; the caller keeps ownership of its buffers.
 * Tables that make an emission +infinity — a level with stdv == 0, a model row with level_stdv == 0 or an infinite lambda =
 * sd_mean^3 / sd_stdv^2, a lik_offset that is not finite — are PS_ERR_BAD_ARG, the message naming the first of them.  Other values
 * outside the reference's domain (NaN or infinite means, negative or infinite deviations) are taken; ps_viterbi_mutate and
 * ps_batch_viterbi_mutate alone answer PS_ERR_BAD_ARG for such an AlignData. */
int ps_align_create(ps_align** out, const char* seq, int64_t seq_len, int32_t n_events,
                    const int64_t* level_off, const double* mean, const double* stdv,
                    const double* ref_align, const double* ref_like, const double* model,
                    const double* trans, const char* evseq, const int64_t* evseq_off,
                    const ps_params* params);
void ps_align_destroy(ps_align* a);
/* `data.params.scoring_width = params['point_width']` (_poreseqcpp.pyx:293-294, 361-362, 465-466). */
int ps_align_set_scoring_width(ps_align* a, int32_t width);
/* A driver that keeps one AlignData alive across several PSAlign calls (events resident in device memory instead of
 * re-marshalled per call) announces each new call with this: it resets what PythonToAlignData would have rebuilt —
 * params.scoring_width and the seed-likelihood cache (cpp/AlignData.h:34), which the reference drops between PSAlign
 * calls (_poreseqcpp.pyx:139-153).  The sequence carries over.  The events' ref_align / ref_like carry over as the Python
 * attributes do in the reference, and those are written only by the calls that end in MakeMutations (ApplyMuts, Mutate,
 * Refine: UpdatePythonEvents, _poreseqcpp.pyx:375, 434, 471).  ScoreEvents, ScorePoints and ScoreMutations realign a scratch
 * AlignData and drop it, so a driver announces such a call with ps_align_new_call + ps_align_keep_refs, and the next
 * ps_align_new_call puts ref_align / ref_like (and what follows from them: ref_index, refstart, refend) back to where that
 * call found them.  Without ps_align_keep_refs the realignment of a scoring call stays in the handle, and with any
 * realign_width that does not bring an event back to the same path the next call starts somewhere a PSAlign never is. */
int ps_align_new_call(ps_align* a, int32_t scoring_width);
/* The call just announced will not write ref_align / ref_like back (no ps_make_mutations follows): remember them as they are
 * now — the last write-back point — for the next ps_align_new_call to restore.  One device copy of the refs the first time
 * after a write-back, nothing while scoring calls follow each other; ps_make_mutations / ps_batch_make_mutations forget the
 * kept refs, and calls that write back (never announced this way) cost nothing extra. */
int ps_align_keep_refs(ps_align* a);
int32_t ps_align_n_events(const ps_align* a);
int64_t ps_align_n_levels(const ps_align* a, int32_t ev);
int64_t ps_align_sequence_length(const ps_align* a);
/* data.sequence.bases (_poreseqcpp.pyx:375, 433, 470); `out` needs sequence_length bytes (no NUL). */
int ps_align_get_sequence(const ps_align* a, char* out, int64_t cap);
/* UpdatePythonEvents (_poreseqcpp.pyx:131-137): copy one event's ref_align / ref_like out. */
int ps_align_get_event_refs(const ps_align* a, int32_t ev, double* ref_align, double* ref_like);

/* ---- vector<MutInfo> / vector<MutScore> (cpp/AlignUtil.h:69-91) ---- */
typedef struct ps_muts ps_muts;
/* orig_off / mut_off are CSR offsets [n+1] into the two byte pools; score may be
 * NULL (then every score is the MutScore seed -1e-6, cpp/AlignUtil.h:86). */
int ps_muts_create(ps_muts** out, int64_t n, const int32_t* start, const int64_t* orig_off,
                   const char* orig_pool, const int64_t* mut_off, const char* mut_pool,
                   const double* score);
void ps_muts_destroy(ps_muts* m);
int64_t ps_muts_count(const ps_muts* m);
int64_t ps_muts_orig_bytes(const ps_muts* m);
int64_t ps_muts_mut_bytes(const ps_muts* m);
int ps_muts_export(const ps_muts* m, int32_t* start, int64_t* orig_off, char* orig_pool,
                   int64_t* mut_off, char* mut_pool, double* score);

/* ---- vector<Sequence> results (ViterbiMutate) ---- */
typedef struct ps_seqs ps_seqs;
void ps_seqs_destroy(ps_seqs* s);
int64_t ps_seqs_count(const ps_seqs* s);
int64_t ps_seqs_bytes(const ps_seqs* s);
int ps_seqs_export(const ps_seqs* s, int64_t* off /*[count+1]*/, char* pool);

/* ---- the five free functions of cpp/Mutations.h:18-24 ---- */

/* ScoreAlignments (cpp/MakeMutations.cpp:148-195): forward fill + backtrace per event;
 * scores[E]; likes (NULL or [sequence_length], accumulated into, as the reference does). */
int ps_score_alignments(ps_align* a, double* scores, double* likes);
/* FindPointMutations (cpp/FindMutations.cpp:191-234). */
int ps_find_point_mutations(ps_align* a, ps_muts** out);
/* FindMutations (cpp/FindMutations.cpp:24-186); seed sequences as a CSR string pool. */
int ps_find_mutations(ps_align* a, int32_t n_seqs, const int64_t* seq_off, const char* seq_pool,
                      ps_muts** out);
/* ScoreMutations (cpp/MakeMutations.cpp:23-69): same order as the input list.  Re-aligns
 * every event as a side effect, as the reference does. */
int ps_score_mutations(ps_align* a, const ps_muts* muts, ps_muts** out_scored);
/* The terms of that sum instead of the sum: deltas[e * n_muts + m] = what event e adds to the score of edit m
 * (cpp/MakeMutations.cpp:51: score[m] = -1e-6 + delta[0][m] + delta[1][m] + ... in event order).  For drivers that shard the
 * EVENTS of one region over several GPUs (second axis): every rank scores its events, the deltas are
 * gathered and every rank adds them up in the reference's order (poreseq_amd.dist.score_mutations_event_sharded).
 * Events are re-aligned as by ps_score_mutations.  deltas needs n_events * n_muts doubles. */
int ps_score_mutation_deltas(ps_align* a, const ps_muts* muts, double* deltas);
/* MakeMutations (cpp/MakeMutations.cpp:74-146): greedy application, returns mutated-base count. */
int ps_make_mutations(ps_align* a, const ps_muts* scored, int32_t* n_bases);

/* Variant.py:48-61 for n_seqs sequences: scores[s * n_events + e] = ScoreEvents()[e] of a copy of the AlignData realigned to
 * sequence s (pyx:241-261, EventData.py:226-256); accuracy[s] = swalign's identity in %.  The AlignData is not modified.
 * All sequences run as one chain: a Smith-Waterman batch whose traceback leaves, per sequence, a partner table on the device (no index
 * list comes back), the events' ref_align re-mapped through it on the device by PSEvent.mapaligns' rule, and (sequence x event) forward
 * alignments in chunks sized by the device-memory plan; identical sequences are aligned and scored once.  A sequence whose alignment
 * with the current one is empty is PS_ERR_BAD_ARG, the message naming its index (the reference dies there with an IndexError).
 * accuracy may be NULL.  Sequences as a CSR string pool, as ps_find_mutations takes its seeds. */
int ps_score_sequences(ps_align* a, int32_t n_seqs, const int64_t* seq_off, const char* seq_pool, double* scores, double* accuracy);

/* The scores of ScorePoints (_poreseqcpp.pyx:278-308, `poreseq variant -a`, Variant.py:77-78) as a table per position instead of a
 * scored list: FindPointMutations' list (cpp/FindMutations.cpp:200-228) is scored as by ps_score_mutations — at the scoring width the
 * AlignData carries, events re-aligned as a side effect — and reduced on the device.  A sequence of L bases has n = max(L - 4, 0)
 * positions (the states of cpp/Sequence.h:64-100): FindPointMutations walks those, the last four bases have no row.
 *   table[p * 9 + slot]   slot 0: deletion of base p; 1-4: substitution by A / C / G / T; 5-8: insertion of A / C / G / T in front of
 *                         it.  Each entry is the score ScoreMutations gives that edit: -1e-6 plus the events' terms added in event
 *                         order (cpp/AlignUtil.h:86, cpp/MakeMutations.cpp:51), bit for bit.  The substitution by the base itself
 *                         is not in the list (cpp/FindMutations.cpp:208-216): its slot holds a quiet NaN.  A base that is none of
 *                         A / C / G / T has all four substitutions.
 *   best[p]               margin: the largest non-NaN entry of the row (the support of the best single-base alternative against the
 *                         called base); slot: the FIRST slot, in slot order, that holds it; n_positive: the row's entries > 0.
 * n must be the AlignData's position count (PS_ERR_BAD_ARG otherwise).  Either output may be NULL: it is then neither produced nor
 * copied back.  One call returns all its results in one device-to-host copy. */
typedef struct ps_point_best {
    double margin;
    int32_t slot;
    int32_t n_positive;
} ps_point_best;
int ps_point_table(ps_align* a, double* table /* [n][9] or NULL */, ps_point_best* best /* [n] or NULL */, int64_t n);

/* Per-edit read support by event group.  The list is scored as by ps_score_mutations — at the scoring width the AlignData carries,
 * events re-aligned once as a side effect — and the per-event terms delta[e][m] (what ps_score_mutation_deltas returns) are reduced
 * on the device; the events x edits matrix never goes to the host.  group[e] in 0 .. n_groups - 1 assigns every event to one of
 * 1 <= n_groups <= 8 groups; the library does not know what a group means (strand, sample, haplotype ...).
 *   scores[m]              the bits of ps_score_mutations: -1e-6 plus all events' terms in event order.  May be NULL.
 *   support[m * n_groups + g]
 *       sum                0.0, then += delta[e][m] for e ascending with group[e] == g: plain FP64 adds over ALL events of the
 *                          group, covering or not (a read's term is not zero outside its aligned span).
 *       cover              the events e of g that SPAN the edit: the event has a positive ref_align entry after the call's
 *                          re-alignment and refstart <= start + 1 <= refend, refstart / refend being the int of its first / last
 *                          positive ref_align entry (cpp/EventData.h:110-169) and start + 1 the column of the 5-mer that begins at
 *                          the edit's first base.  This is a span test, not a likelihood test: a covering read's term can be zero.
 *       pos / neg          those of the covering events with delta > 0 / delta < 0.
 *       reserved           0.
 * An edit that ScoreMutations skips (start > sequence length, cpp/MakeMutations.cpp:46-47) has all-zero records and score -1e-6.
 * n_groups outside 1 .. 8, a group id outside 0 .. n_groups - 1 or a NULL group / support is PS_ERR_BAD_ARG.  An empty list is PS_OK
 * and launches nothing (the events are then not re-aligned either).  One call, or one chunk of a batch that was cut to fit device
 * memory, returns all its results in one device-to-host copy. */
typedef struct ps_edit_support {
    double sum;
    int32_t cover, pos, neg, reserved /* 0 */;
} ps_edit_support;   /* 24 bytes */
int ps_score_mutation_support(ps_align* a, const ps_muts* muts, int32_t n_groups, const int32_t* group /* [n_events] */,
                              double* scores /* [M] or NULL */, ps_edit_support* support /* [M][n_groups] */);

/* Genotype likelihoods per edit.  ps_score_mutation_support's call — same list, same scoring, same re-alignment, same group
 * arguments and checks — with a second reduction of the same events x edits matrix on the device (k_genotype).  ps_score_mutations
 * adds an edit's terms over all reads: the log-likelihood of "every read carries the edit".  A genotype whose alt-allele fraction
 * is f has  sum over reads of log((1 - f) + f * exp(delta))  instead.
 *   alt_frac[k]            0 <= n_frac <= 8 alt fractions, each 1e-6 <= f <= 1 - 1e-6;  g_k = 1.0 - f_k is formed once on the host.
 *   cover(e, m)            exactly the test behind ps_edit_support.cover: the edit is not skipped (start <= sequence length), event e
 *                          has a positive ref_align entry after the call's re-alignment and refstart <= start + 1 <= refend.
 *                          ONLY covering events enter the likelihoods: a read's term is not zero outside its span, and such terms
 *                          are noise here.
 *   n_cover[m]             the number of covering events.  May be NULL.
 *   lik[m * (n_frac + 1) + k], k < n_frac
 *                          acc = 0.0; for e ascending with cover(e, m):  d = delta[e][m];  u = exp(-|d|);
 *                          x = (d > 0) ? g_k * u + f_k : g_k + f_k * u;  acc += (d > 0 ? d : 0.0) + log(x).
 *                          One exp per (event, edit), one log per fraction, no argument of exp is positive and x lies in
 *                          [min(f, 1 - f), 1]: nothing overflows.  d = -inf contributes log(g_k), d = +inf gives +inf, NaN gives NaN.
 *                          exp / log are the device library's FP64 functions: these columns agree with a host evaluation to a few
 *                          units in the last place per term, not bit for bit.
 *   lik[m * (n_frac + 1) + n_frac]
 *                          0.0, then += d over the covering events in event order, plain FP64 adds: the hom-alt likelihood, bit-exact.
 *                          (The hom-ref likelihood is 0 by construction and is not stored.)
 *   scores[m]              the bits of ps_score_mutations.  May be NULL.
 *   support                as ps_score_mutation_support; may be NULL here and is then neither produced nor copied.
 * A skipped edit, and every edit of an AlignData without events, has n_cover = 0 and all-zero lik.  PS_ERR_BAD_ARG: n_frac outside
 * 0 .. 8, a fraction outside 1e-6 .. 1 - 1e-6 (NaN included), NULL alt_frac with n_frac > 0, NULL lik, and what the support call
 * rejects.  An empty list is PS_OK and launches nothing.  Scores, records, lik and n_cover of one call (or chunk) come back in the
 * one device-to-host copy of the support call.  Uncalibrated, like everything derived from these scores. */
int ps_score_mutation_genotypes(ps_align* a, const ps_muts* muts, int32_t n_groups, const int32_t* group /* [n_events] */,
                                int32_t n_frac, const double* alt_frac /* [n_frac]; NULL allowed when n_frac == 0 */,
                                double* scores /* [M] or NULL */, ps_edit_support* support /* [M][n_groups] or NULL */,
                                double* lik /* [M][n_frac + 1] */, int32_t* n_cover /* [M] or NULL */);

/* Phase of heterozygous edits.  The list of candidate sites (a driver passes its het calls sorted by position; the library takes
 * any list, and "order" below is list order) is scored as by ps_score_mutations — same re-alignment side effect, same checks — and
 * the events x edits matrix delta[e][m] is then reduced three times on the device (k_link, k_phase, k_haptag).  cover(e, m) is
 * exactly the test of ps_edit_support.cover / ps_score_mutation_genotypes.  E events, M sites, window W, S = max_sets.
 *
 *   link[m * W + (w - 1)]  the pair (m, j = m + w), w = 1 .. W; all zero where j >= M.  For e ascending over the events with
 *                          cover(e, m) && cover(e, j), da = delta[e][m], db = delta[e][j], s = da + db, r = da - db:
 *       cis               += (s > 0 ? s : 0.0) + log(0.5 + 0.5 * exp(-fabs(s)))       sum log(1/2 e^(da + db) + 1/2): both alts on one copy
 *       trans             += (da > db ? da : db) + log(0.5 + 0.5 * exp(-fabs(r)))     sum log(1/2 e^da + 1/2 e^db): one alt on each copy
 *       n_both            ++
 *       n_cis             += (da > 0 && db > 0) || (da < 0 && db < 0)
 *       n_trans           += (da > 0 && db < 0) || (da < 0 && db > 0)
 *                          No argument of exp is positive and every argument of log lies in [0.5, 1]; non-finite terms give what IEEE
 *                          gives for these lines.  exp / log are the device library's FP64 functions: cis / trans agree with a
 *                          host evaluation to a few units in the last place per term, not bit for bit.
 *   phase[m]               a serial scan in list order, defined on the link records alone (a host can replay it bit for bit):
 *                          site 0 has vote = 0.0, hap = +1, set = 0.  Site m > 0: vote = 0.0; for w = 1 .. min(W, m) ascending with
 *                          i = m - w and L = link[i * W + (w - 1)]:  if phase[i].set == phase[m - 1].set && L.n_both > 0 then
 *                          vote += phase[i].hap * (L.cis - L.trans), plain FP64 operations in that order.  If vote != 0.0 &&
 *                          fabs(vote) >= min_link (a NaN fails both) site m joins: set = phase[m - 1].set, hap = vote > 0 ? +1 : -1.
 *                          Otherwise it opens a new set: set = phase[m - 1].set + 1, hap = +1.  vote is stored either way.
 *                          hap = +1: the site's alt is on the copy that carries the alt of the set's first site.
 *   n_sets                 phase[M - 1].set + 1 (0 for an empty list).  May be NULL.
 *   hap[e * S + k]         event e against the k-th phase set (sets with ordinal >= S are not tagged): lik1 / n1 the sum and the count
 *                          over the sites m of set k with cover(e, m) and hap == +1, lik2 / n2 the same for hap == -1.  The order of
 *                          the adds is fixed: partial l = 0.0, then += delta[e][m] for m = l, l + 64, l + 128, ... ascending (sites
 *                          that do not qualify are passed over), and the 64 partials are added into 0.0 for l = 0 .. 63.  An event
 *                          is from the first copy where lik1 > lik2.  May be NULL: then neither produced nor copied.
 *   scores[m]              the bits of ps_score_mutations.  May be NULL.
 * An AlignData without events gets the records the rules give for all-zero links, written on the host: every site its own set, hap
 * +1, vote 0.0, n_sets = M, scores -1e-6; hap then has no rows.  A skipped edit is covered by no event.  An empty list is PS_OK and
 * launches nothing; n_sets is then 0 and hap all zero.  PS_ERR_BAD_ARG: window outside 1 .. 8, max_sets outside 1 .. 8, min_link
 * negative or not finite (NaN included), NULL link or phase, and what ps_score_mutations rejects.  All outputs of one call, or of one
 * chunk of a batch that was cut to fit device memory, come back in one device-to-host copy; a batch is cut between AlignData, never
 * inside a list.
 * Model limit: an edit's terms are treated as independent of the other edit of the pair.  For two edits closer than the scoring band
 * this is an approximation (a read's term for one edit is computed on the sequence without the other).  Votes, sets and haplotypes
 * are uncalibrated, like everything derived from these scores. */
#define PS_LINK_MAX_WINDOW 8
#define PS_PHASE_MAX_SETS 8
typedef struct ps_edit_link {
    double cis, trans;
    int32_t n_both, n_cis, n_trans, reserved /* 0 */;
} ps_edit_link;    /* 32 bytes */
typedef struct ps_edit_phase {
    double vote;
    int32_t hap /* +1 / -1 */, set;
} ps_edit_phase;   /* 16 bytes */
typedef struct ps_event_hap {
    double lik1, lik2;
    int32_t n1, n2;
} ps_event_hap;    /* 24 bytes */
int ps_score_mutation_phase(ps_align* a, const ps_muts* muts, int32_t window, double min_link, int32_t max_sets,
                            double* scores /* [M] or NULL */, ps_edit_link* link /* [M][window] */, ps_edit_phase* phase /* [M] */,
                            ps_event_hap* hap /* [n_events][max_sets] or NULL */, int32_t* n_sets /* one, or NULL */);

/* Alignment census and the sums of a shift / scale refit, per event, reduced on the device from the alignment the handle holds
 * (k_align_stats).  The pore model of every read arrives scaled by numbers that were fitted before the read was aligned to
 * anything (EventData.py:140-168); with an event-to-sequence alignment in hand they can be refitted by weighted least squares of
 * the level means against the model means of the states they aligned to.  The library returns the sufficient statistics; the fit
 * itself is six lines on the host (poreseq_amd.util.fit_scaling).
 *
 * realign != 0 runs exactly ps_score_alignments' chain first — forward fill, then backtrace per event — and `scores` (may be NULL)
 * gets the bits ps_score_alignments returns.  The realignment stays in the handle as after any scoring call (a resident driver
 * announces the call with ps_align_new_call + ps_align_keep_refs); the records are reduced from the refs the backtrace just wrote,
 * in the same launch chain, and scores and records come back in one device-to-host copy.
 * realign == 0 reduces the refs the handle holds now and launches no DP; `scores` must then be NULL (PS_ERR_BAD_ARG otherwise).
 * A NULL `stats` is PS_ERR_BAD_ARG.  An AlignData without events is PS_OK and launches nothing.
 *
 * One event's record.  The event has n levels with ra[i] (ref_align) and mean[i]; the sequence has S states, states[j - 1]
 * belonging to DP column j (cpp/Alignment.cpp:125); the event's model rows are m_k = level_mean[k], s_k = level_stdv[k].
 *   A level is ALIGNED iff ra[i] > 0 (the test of cpp/EventData.h:121), INSERTED iff ra[i] < 0, UNALIGNED otherwise (0, NaN); its
 *   column is c = (int)fmin(ra[i], 2147483647.0).  n_levels = n; n_aligned, n_insert, n_unaligned count the three kinds.
 *   first_col / last_col   the columns of the first and the last aligned level, both 0 when there is none.
 *   Census.  Walk in level order carrying p, the column of the previous ALIGNED level, and prev_rep; inserted and unaligned
 *       levels in between change neither.  An aligned level with a predecessor has d = c - p:  d == 0: n_extend++ if prev_rep,
 *       else n_stay++;  d == 1: n_step++;  d > 1: n_jump++ and n_gap_cols += d - 1;  d < 0: n_back++.  Then prev_rep = (d == 0).
 *       The first aligned level sets prev_rep = false.
 *       The census is of the ref ARRAY, not of the path's moves: a -1 level is either U_INSERT or UL_IGNORE
 *       (cpp/Alignment.cpp:559-573) and the array cannot tell them apart; a "stay" here is a repeated column, whatever move made it.
 *   Fit terms.  An aligned level with 1 <= c <= S and k = states[c - 1] >= 0 enters the fit and counts in n_fit; any other aligned
 *       level (a column past the sequence, a column 0 from an entry in (0, 1), a 5-mer with a base outside ACGT) counts in n_nostate.
 *       For a level that enters, every operation rounded once (IEEE double, no contraction):
 *           w = 1.0 / (s_k * s_k);  wm = w * m_k;  r = mean[i] - m_k;
 *           sw += w;  swm += wm;  swmm += wm * m_k;  swr += w * r;  swmr += wm * r;  swrr += (w * r) * r.
 *   Order of the adds (a host can reproduce the bits, as for ps_event_hap): partial t = +0.0 takes the qualifying levels
 *       i = t, t + 256, t + 512, ... ascending; the 256 partials are then added into +0.0 for t = 0 .. 255.
 * The batch form is one launch for all regions; a batch whose realignment does not fit device memory is cut between AlignData,
 * never inside one.  Not part of the reference's interface.  Not built: drift (the ABI carries no level times) and sd_stdv per
 * k-mer.  The stdv channel's scale_sd / var_sd and per-k-mer model re-estimation are fitted from ps_kmer_stats' tables, the
 * transition parameters from the backtrace's moves, which the array cannot carry: ps_move_stats (both below). */
typedef struct ps_event_stats {
    int32_t n_levels, n_aligned, n_insert, n_unaligned;
    int32_t n_step, n_stay, n_extend, n_jump, n_back;
    int32_t n_nostate, n_fit, first_col, last_col, reserved /* 0 */;
    int64_t n_gap_cols;
    double sw, swm, swmm, swr, swmr, swrr;
} ps_event_stats;   /* 112 bytes, no padding */
int ps_align_stats(ps_align* a, int32_t realign, double* scores /* [E] or NULL */, ps_event_stats* stats /* [E] */);

/* Per-k-mer model statistics by event group, reduced on the device from the alignment the handle holds (k_kmer_stats): for every
 * group of events and every one of the 1024 5-mer states the sufficient statistics of a re-estimation of that state's model rows —
 * level mean and variance, the stdv channel's mean — and, summed over the states, of the stdv channel's scale_sd / var_sd.  The
 * fits are a few lines on the host (poreseq_amd.util.fit_kmers, fit_scaling_sd).
 *
 * `realign` and `scores` are ps_align_stats': realign != 0 runs ps_score_alignments' chain first, `scores` (may be NULL) gets its
 * bits and the realignment stays in the handle; realign == 0 reduces the refs the handle holds, launches no DP, and `scores` must
 * be NULL (PS_ERR_BAD_ARG otherwise).  groups[e] is the group of event e, 0 .. n_groups - 1, n_groups is 1 .. 256
 * (PS_KMER_MAX_GROUPS); table has n_groups rows of 1024 records (ps_kmer_cell), row g for group g.  PS_ERR_BAD_ARG: n_groups outside 1 .. 256,
 * an id outside 0 .. n_groups - 1, a NULL table, NULL groups with events.  An AlignData without events is PS_OK, launches nothing
 * and gets an all-zero table; a group without events has all-zero rows.
 *
 * Which levels enter is ps_align_stats' n_fit rule: a level with ra[i] > 0 whose column c = (int)fmin(ra[i], 2147483647.0) has
 * 1 <= c <= S and whose state k = states[c - 1] lies in 0 .. 1023.  With the event's model rows m_k = level_mean[k], s_k =
 * level_stdv[k], mu_k = sd_mean[k] and lam_k = sd_lambda[k] (= sd_mean^3 / sd_stdv^2), every operation rounded once (IEEE double,
 * no contraction):
 *     z = (mean[i] - m_k) / s_k;  u = stdv[i] / mu_k;  p = lam_k / mu_k;
 *     n += 1;  sz += z;  szz += z * z;  sp += p;  spu += p * u;  spv += p / u          into table[groups[e]][k].
 * Order of the adds (a host can reproduce the bits): every sum of one (g, k) starts at +0.0 and is serial — the events of group g
 * in event order, within an event the levels in ascending order.  Non-finite inputs propagate by IEEE rules into the cells they
 * touch and nowhere else.
 * Invariant: the sum of n over a table equals the sum of n_fit of ps_align_stats' records on the same refs.
 * The batch form is one launch of k_kmer_stats for all regions and one copy back; a batch whose realignment or whose tables do not
 * fit device memory is cut between AlignData, never inside one.  Not part of the reference's interface. */
#define PS_KMER_MAX_GROUPS 256
typedef struct ps_kmer_cell {
    int64_t n;
    double sz, szz, sp, spu, spv;
} ps_kmer_cell;   /* 48 bytes, no padding (C has one name space for types and functions: the record cannot carry the call's name) */
int ps_kmer_stats(ps_align* a, int32_t realign, const int32_t* groups /* [E] */, int32_t n_groups,
                  double* scores /* [E] or NULL */, ps_kmer_cell* table /* [n_groups][1024] */);

/* The moves of the backtrace, per event, counted on the device (k_move_stats): what a fit of the transition probabilities
 * skip / stay / extend / insert needs and ref_align cannot carry — the backtrace writes -1 for U_INSERT and UL_IGNORE alike
 * (cpp/Alignment.cpp:559-573), a repeated column does not say whether U_STAY or U_EXTEND made it, and a skipped column next to
 * an inserted level is ambiguous.  The fit is a few lines on the host (poreseq_amd.util.fit_transitions).
 *
 * The call always realigns: it is ps_score_alignments' chain, bit for bit — forward fill, then backtrace per event — with one
 * more kernel between the walk and the kernel that turns the walk's records into ref_like.  `scores` (may be NULL) gets the bits
 * ps_score_alignments returns; ref_align and ref_like stay in the handle as after any scoring call (a resident driver announces
 * the call with ps_align_new_call + ps_align_keep_refs, as for ps_align_stats with realign != 0); records, per-level arrays and
 * scores come back in one device-to-host copy.  A NULL `moves` is PS_ERR_BAD_ARG.  An AlignData without events is PS_OK and
 * launches nothing.  An AlignData marked non-finite runs like every scoring call.
 *
 * One event's record.  The walk (cpp/Alignment.cpp:537-605) starts on the forward matrix' best cell (top_level, top_col) =
 * (maxScore.i, maxScore.j), both 0 when the best score is not > 0, and steps until it reaches row 0 or a cell whose score is
 * <= 0 (end_kind 0) or a cell whose step is Z_IMPLICIT (end_kind 1); low_col is the column of that cell, which the walk does
 * not record.  Every step but L_SKIP and the change from the main to the stay matrix records one level; the levels recorded are
 * low_level .. top_level without a hole (low_level = 0 and all counts 0 when there is none).
 *   n_match, n_ignore, n_insert, n_stay, n_extend   recorded levels by the step that recorded them: UL_MATCH, UL_IGNORE, U_INSERT,
 *       U_STAY (taken in the stay matrix), U_EXTEND.
 *   Skips.  Between the record of level i (column j_i) and that of level i - 1 the walk takes (j_i - dj_i) - j_(i-1) L_SKIP steps,
 *       dj = 1 for MATCH / IGNORE and 0 for INSERT / STAY / EXTEND; above the record of top_level it takes top_col - j_top, below
 *       that of low_level (j_low - dj_low) - low_col.  Each of these that is > 0 is one maximal run: n_skip_runs counts them,
 *       max_skip is the longest, n_skip_cols their sum.
 *   inert   the reference's stripe_width == 0 for this call (realign_width 0, or no aligned level): the refs were left alone,
 *       n_levels is the event's level count and every other field is 0.
 * Per level, when asked for: step[e][i] is the reference's move code of the step that recorded level i + 1 — 1 MATCH, 2 INSERT,
 * 3 IGNORE, 4 STAY, 5 EXTEND — and 0 for a level not on the path (L_SKIP records nothing); col[e][i] is the column of the cell it
 * was recorded from, also for INSERT and IGNORE where ref_align says -1, and 0 off the path.  `step` and `col` are arrays of
 * n_events pointers, entry e to n_levels(e) elements (an entry may be NULL for an event without levels); either may be NULL.
 * Invariants:
 *   n_match + n_ignore + n_insert + n_stay + n_extend == top_level - low_level + 1   when a level was recorded;
 *   n_match + n_ignore + n_skip_cols == top_col - low_col;
 *   against the ps_event_stats record of the refs the same call leaves, for a record that is not inert:
 *       n_match + n_stay + n_extend == n_aligned   and   n_ignore + n_insert == n_insert there.
 * Counts are integers and max_skip is a maximum: no order of the adds to define.  The batch form is one launch chain with one
 * launch of k_move_stats and one copy back; a batch whose matrices do not fit device memory is cut between AlignData, never
 * inside one.  Not part of the reference's interface.  Not built: a fit of lik_offset. */
typedef struct ps_event_moves {
    int32_t n_levels, inert;
    int32_t top_level, top_col;
    int32_t low_level, low_col;
    int32_t end_kind;
    int32_t n_match, n_ignore, n_insert, n_stay, n_extend;
    int32_t n_skip_runs, max_skip;
    int64_t n_skip_cols;
} ps_event_moves;   /* 64 bytes, no padding */
int ps_move_stats(ps_align* a, double* scores /* [E] or NULL */, ps_event_moves* moves /* [E] */,
                  uint8_t* const* step /* [E] of [n_e], or NULL */, int32_t* const* col /* [E] of [n_e], or NULL */);

/* Posterior move counts: the sum over ALL alignments in an event's band, and the expected number of each move under it — where
 * ps_move_stats counts the moves of the one best path.  No backtrace runs and nothing of the handle changes: ref_align, ref_like,
 * what ps_align_keep_refs keeps and the host copies stay what they were.
 *
 * The lattice is the forward fill's own, for an event on the refs it carries when the call begins:
 *   columns j = 1 .. C, C = n_states; band rows i0(j) .. i1(j) of cpp/Alignment.cpp:127-148 with stripe_width = realign_width
 *       (exactly the non-NaN pattern of ps_debug_fill, direction 0); the blank column 0 with rows 0 .. n0;
 *   obs(i, j) the fill's emission, lik_offset and the log_stdv[n0 - i] quirk (cpp/Alignment.cpp:169-173) included.
 * The recursion is the reference's (cpp/Alignment.cpp:189-267) with every max / > chain replaced by log-sum-exp, (+):
 *   the blank column and every column whose state is < 0 (calloc'd, returned early): M = S = 0 on all their rows.  These cells are
 *       constants: nothing flows through them, and they are not part of logz.
 *   S(i, j) = 0 (+) (M(i-1, j) + obs + lik_stay) (+) (S(i-1, j) + obs + lik_extend)   for i > i0(j); the 0 is the calloc'd floor.
 *   S(i0, j) = -infinity.
 *   M(i, j) = 0 (+) skip (+) match (+) ignore (+) insert (+) S(i, j), with ONE floor term 0, and with p0 .. p1 the previous
 *       column's band and Mp its M:
 *       skip   = Mp(i) + lik_skip;
 *       match  = Mp(i-1) + obs;
 *       ignore = Mp(i-1) + lik_insert, present only when p0 < i <= p1;
 *       insert = M(i-1, j) + lik_insert, present only when i > i0;
 *       Mp(r) is the previous column's M(r) when the row tested lies in its band — p0 <= i <= p1 for skip, p0 < i <= p1 for
 *       match — and the implicit 0 otherwise (cpp/Alignment.cpp:200-225).  An absent candidate adds nothing.
 *   logz = (+) of M(i, j) over all band cells of the columns with a valid state; an event without such a cell has logz = 0 and
 *       all counts 0.
 *   e_skip, e_match, e_ignore, e_insert, e_stay, e_extend: for each move the sum over cells of exp(F(pred) + w + beta(cell) -
 *       logz), F(pred) the forward value the move starts from (0 for a constant or implicit one: implicit skips and matches are
 *       counted), w the move's term, beta the adjoint (backward) quantity of the same lattice — the log-sum of what follows a
 *       cell, with the 1 of "the path ends here" in M of the columns with a state: beta_M(c) = 0 (+) the moves out of M(c),
 *       beta_S(c) = beta_M(c) (+) the extend out of S(c).
 *   n_cells the band cells of the columns with a valid state, n_cols those columns.
 *   Per level, when asked for: emit[e][i-1] the expected number of emitting arrivals (match + stay + extend, over all columns) at
 *       level i, col[e][i-1] their posterior mean column (NaN where emit is 0).  `emit` and `col` are arrays of n_events pointers,
 *       entry e to n_levels(e) doubles (an entry may be NULL for an event without levels); both NULL, or both given.
 *   inert   ps_move_stats' rule (realign_width 0, no aligned level, no level at all): n_levels is the event's level count, every
 *       other field 0 and the event's per-level arrays are not written.
 * FP64, log domain; sums run in a fixed order (per lane, then lanes in order): two runs give the same bytes.  A band footprint of
 * more than 1024 rows on one anti-diagonal (realign_width > 511 on a long read) is PS_ERR_UNSUPPORTED, an AlignData marked
 * non-finite PS_ERR_BAD_ARG, as for ps_viterbi_mutate; the handle stays usable.  A batch whose tables — (n0 + C + 25) x slots x 16
 * bytes per event — exceed the calling thread's share of the device is cut between AlignData; one AlignData over the share is
 * PS_ERR_NOMEM.  Not part of the reference's interface.  Not built: posterior-weighted k-mer statistics, a fit of lik_offset. */
typedef struct ps_event_posterior {
    int32_t n_levels, inert, n_cols, pad;
    int64_t n_cells;
    double logz, e_skip, e_match, e_ignore, e_insert, e_stay, e_extend;
} ps_event_posterior;   /* 80 bytes, no padding */
int ps_posterior_stats(ps_align* a, ps_event_posterior* stats /* [E] */, double* const* emit /* [E] of [n_e], or NULL */,
                       double* const* col /* [E] of [n_e], or NULL */);

/* ViterbiMutate (cpp/Viterbi.h:67-68, cpp/Viterbi.cpp:239-426).  The nkeep > 0 stochastic back-traces draw
 * rand() / (RAND_MAX + 1.0) in the reference's call order (cpp/Viterbi.cpp:108).  The reference never seeds
 * libc rand() and runs one process per region, so every region sees the generator of a fresh process.  The
 * HIP library keeps that contract per host thread: each thread owns a glibc random_r() state (the TYPE_3
 * additive-feedback generator rand() itself uses), initially seeded with 1 like an unseeded process, without
 * the process-wide lock behind rand() that serialises concurrent regions.  ps_srand re-seeds the calling
 * thread's generator (srand(seed) in the oracle / reference builds of this ABI).
 *
 * nkeep == 0 asks for the one deterministic back-trace: p[T-1] = the first maximum of the final scores, p[i-1] = bp[i][p[i]] over
 * the T kept positions.  The recursion starts every maximum at -1e300 with back-pointer -1, so a kept position where every state's
 * emission is -inf or below -1e300, or where the running scores have passed -1e300, leaves -1 in all 1024 states, and so does every
 * later one.  Finite, unmarked data gets there (a level mean or deviation near 1e151 or above).  Where some bp[i][p[i]], i >= 1, is
 * -1 there is no path: ps_viterbi_mutate, ps_batch_viterbi_mutate, ps_debug_viterbi and ps_debug_viterbi_steps answer
 * PS_ERR_BAD_ARG, the message naming the entry point, the region index of a lock-step call and the first such kept position
 * ("ps_batch_viterbi_mutate: region 1: no state is reachable at kept position 100 (...)").  A lock-step call with one such region
 * is refused as a whole; the AlignData stays usable for every other call.  bp[0] is never followed, so T = 1 always has a path.
 * The stochastic back-traces (nkeep > 0) do not read back-pointers and run on such tables as the reference does.  (The reference
 * itself indexes with the -1 here; the reference shim of this ABI is not to be called with nkeep == 0 on such data.) */
int ps_srand(uint32_t seed);
/* The next n deviates rand() / (RAND_MAX + 1.0) of the calling thread's generator (consumes them). */
int ps_rand_draw(int64_t n, double* out);
int ps_viterbi_mutate(ps_align* a, int32_t nkeep, double skip_prob, double stay_prob,
                      double mut_min, double mut_max, int32_t verbose, ps_seqs** out);

/* ---- lock-step batches over independent AlignData ----------------------------------------------------------------
 * The reference refines one region per process (cmdline.py:182-195, split_fasta.py:50-133); regions are independent.
 * One region keeps a few percent of an MI355X busy, so a driver that has several regions in hand runs the SAME call
 * for all of them through these entry points: every phase (Smith-Waterman batch, banded fills, edit scoring, Viterbi)
 * becomes one launch chain over all regions' events, from one host thread, on the library's own stream.  Results are
 * those of the single-handle calls on each AlignData, bit for bit.  Arrays have n entries; handles must be distinct.
 *
 * ps_rng: the generator ViterbiMutate's stochastic back-traces draw from (rand() of cpp/Viterbi.cpp:108).  The
 * reference's process-per-region model gives every region the stream of a fresh process, continued across the
 * region's Viterbi calls; a lock-step driver therefore keeps one ps_rng per region (seed 1 = unseeded process). */
typedef struct ps_rng ps_rng;
int ps_rng_create(ps_rng** out, uint32_t seed);
void ps_rng_destroy(ps_rng* r);
/* vector<Sequence> from a CSR string pool (seed sequences for ps_batch_find_mutations). */
int ps_seqs_create(ps_seqs** out, int64_t n, const int64_t* off, const char* pool);
/* ScoreAlignments for n AlignData: scores[i] has n_events(i) entries, likes[i] is NULL or [sequence_length(i)]. */
int ps_batch_score_alignments(int32_t n, ps_align* const* a, double* const* scores, double* const* likes);
/* FindMutations: seeds[i] are the candidate sequences of AlignData i; out[i] receives a new ps_muts. */
int ps_batch_find_mutations(int32_t n, ps_align* const* a, const ps_seqs* const* seeds, ps_muts** out);
/* ScoreMutations: out[i] receives a new ps_muts with the scores of muts[i], same order. */
int ps_batch_score_mutations(int32_t n, ps_align* const* a, const ps_muts* const* muts, ps_muts** out);
/* MakeMutations: greedy application per AlignData; the re-scoring rounds of the recursion are batched. */
int ps_batch_make_mutations(int32_t n, ps_align* const* a, const ps_muts* const* scored, int32_t* n_bases);
/* `poreseq variant -v` for every AlignData: seqs[i] are the candidate sequences of AlignData i (ps_seqs_create), scores[i] has
 * count(seqs[i]) * n_events(i) doubles and accuracy[i] (or the whole array) may be NULL: ps_score_sequences for all of them in one chain. */
int ps_batch_score_sequences(int32_t n, ps_align* const* a, const ps_seqs* const* seqs, double* const* scores, double* const* accuracy);
/* ps_point_table for every AlignData in one launch chain (the dense ScoreMutations path of Refine) and ONE copy back: table[i] is NULL
 * or [n[i]][9], best[i] NULL or [n[i]] (either array itself may be NULL), n[i] the position count of AlignData i. */
int ps_batch_point_table(int32_t n_regions, ps_align* const* a, double* const* table, ps_point_best* const* best, const int64_t* n);
/* ps_score_mutation_support for every AlignData in one launch chain: muts[i], n_groups[i], group[i] ([n_events(i)]) and support[i] ([count(muts[i])][n_groups[i]]) per AlignData; scores[i], or the whole array, may be NULL. */
int ps_batch_score_mutation_support(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* n_groups /* [n] */,
                                    const int32_t* const* group, double* const* scores /* entries or array may be NULL */,
                                    ps_edit_support* const* support);
/* ps_score_mutation_genotypes for every AlignData in one launch chain: n_frac[i], alt_frac[i] ([n_frac[i]]; may be NULL where n_frac[i] == 0) and lik[i] ([count(muts[i])][n_frac[i] + 1]) per AlignData; scores, support and n_cover — entries or whole arrays — may be NULL. */
int ps_batch_score_mutation_genotypes(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* n_groups /* [n] */,
                                      const int32_t* const* group, const int32_t* n_frac /* [n] */, const double* const* alt_frac,
                                      double* const* scores, ps_edit_support* const* support, double* const* lik, int32_t* const* n_cover);
/* ps_score_mutation_phase for every AlignData in one launch chain: window[i], min_link[i], max_sets[i], link[i] ([count(muts[i])][window[i]]) and phase[i] ([count(muts[i])]) per AlignData; scores, hap ([n_events(i)][max_sets[i]]) and n_sets (one int32 each) — entries or whole arrays — may be NULL. */
int ps_batch_score_mutation_phase(int32_t n, ps_align* const* a, const ps_muts* const* muts, const int32_t* window /* [n] */,
                                  const double* min_link /* [n] */, const int32_t* max_sets /* [n] */, double* const* scores,
                                  ps_edit_link* const* link, ps_edit_phase* const* phase, ps_event_hap* const* hap, int32_t* const* n_sets);
/* ps_align_stats for every AlignData in one launch chain and ONE copy back: stats[i] has n_events(i) records (never NULL, also for an AlignData without events); with realign != 0 scores[i] — entries or the whole array may be NULL — has n_events(i) entries, with realign == 0 every scores[i] must be NULL. */
int ps_batch_align_stats(int32_t n, ps_align* const* a, int32_t realign, double* const* scores, ps_event_stats* const* stats);
/* ps_kmer_stats for every AlignData in one launch chain, ONE launch of k_kmer_stats and one copy back: groups[i] has n_events(i) ids (may be NULL for an AlignData without events), n_groups[i] is 1 .. 256, table[i] has n_groups[i] x 1024 records (never NULL); scores as in ps_batch_align_stats. */
int ps_batch_kmer_stats(int32_t n, ps_align* const* a, int32_t realign, const int32_t* const* groups, const int32_t* n_groups /* [n] */,
                        double* const* scores, ps_kmer_cell* const* table);
/* ps_move_stats for every AlignData in one launch chain, ONE launch of k_move_stats and one copy back: moves[i] has n_events(i) records (never NULL, also for an AlignData without events); scores[i] — entries or the whole array may be NULL — has n_events(i) entries; step[i] / col[i] — entries or whole arrays may be NULL — are ps_move_stats' arrays of n_events(i) pointers. */
int ps_batch_move_stats(int32_t n, ps_align* const* a, double* const* scores, ps_event_moves* const* moves,
                        uint8_t* const* const* step, int32_t* const* const* col);
/* ps_posterior_stats for every AlignData in one launch chain — the band stage, k_post_fwd, k_post_bwd — and one copy back: stats[i] has n_events(i) records (never NULL, also for an AlignData without events); emit[i] / col[i] — whole arrays may be NULL, both or neither — are ps_posterior_stats' arrays of n_events(i) pointers. */
int ps_batch_posterior_stats(int32_t n, ps_align* const* a, ps_event_posterior* const* stats, double* const* const* emit,
                             double* const* const* col);
/* ViterbiMutate: rng[i] may be NULL (the calling thread's generator, as ps_viterbi_mutate). */
int ps_batch_viterbi_mutate(int32_t n, ps_align* const* a, ps_rng* const* rng, int32_t nkeep, double skip_prob,
                            double stay_prob, double mut_min, double mut_max, ps_seqs** out);

/* swfull (cpp/swlib.h:36, cpp/swlib.cpp:211-340).  inds1/inds2 need room for n1+n2 entries. */
int ps_swfull(const char* seq1, int64_t n1, const char* seq2, int64_t n2, int32_t* score,
              double* accuracy, int32_t* inds1, int32_t* inds2, int64_t cap, int64_t* n_pairs);
/* swfull for n pairs in one call, each reduced to what the reference's consensus driver reads off the index lists (cpp/swlib.cpp:211-340;
 * poreseq/Mutate.py:59-68 picks its `test` start from the first and last aligned pair, Mutate.py:96-98 counts the zero entries): the
 * pairs run as batched launches cut by the device-memory plan, near-identical pairs banded, and no index list is stored or copied.
 * Per pair, in terms of ps_swfull's inds1 / inds2: n_pairs their length, n_match the matching aligned pairs, first1 / first2 entry 0
 * (0, 0 for an empty alignment), last1 / last2 entry n_pairs - 1, gap1 / gap2 the entries with inds1 == 0 / inds2 == 0,
 * accuracy = 100.0 * n_match / n_pairs as ps_swfull forms it (NaN for an empty alignment). */
typedef struct ps_sw_summary {
    int32_t score, n_pairs, n_match, first1, first2, last1, last2, gap1, gap2;
    double accuracy;
} ps_sw_summary;
int ps_batch_sw_summary(int64_t n, const char* const* seq1, const int64_t* n1, const char* const* seq2, const int64_t* n2,
                        ps_sw_summary* out);
/* Sequence::populateStates (cpp/Sequence.h:64-100); states needs max(n-4,0) entries. */
int ps_seq_to_states(const char* seq, int64_t n, int32_t* states, int64_t* n_states);

/* ---- scratch poison (a test hook; nothing in the library calls it and no environment variable enables it) ----
 * Pools, dense slabs, cached AlignData slabs and pinned staging memory are scratch between API calls.  This
 * hook drains the calling thread's streams and then overwrites, over its whole capacity, everything that thread's next call could
 * find left over: every named device pool of its runtime, every dense slab no call holds, every cached AlignData slab (after its
 * pending event), the pinned host buffers and the staging arena.  A live AlignData's own slab, a busy dense slab and other
 * threads' runtimes are not touched.  index_word goes into every 32-bit word of every buffer that may hold an index, offset, count,
 * flag, state id or loop bound (the default class); value_word into every double of the pools that csrc/ps_poison.h lists as
 * VALUE: scores that are only compared, added and copied.  Pass an index word that is in range wherever one is used (1) and the
 * results of a correct library do not change.  report (may be NULL when cap is 0) gets one record per buffer name, at most cap of
 * them; n_report (may be NULL) the number there are.  Names: a pool's own; "host:<name>" for a pinned host buffer; "slab" (all dense
 * slabs, skipped = the busy ones), "align_cache", "stage".  The checker libraries do not export it. */
typedef struct ps_poison_report {
    char name[32];
    int64_t bytes;      /* bytes overwritten; 0: not allocated, or skipped */
    int32_t cls;        /* 0 index word, 1 value word, 2 exempt (carries state between calls on purpose: left alone) */
    int32_t skipped;    /* buffers of this name that were left alone: busy dense slabs, an exempt pool */
} ps_poison_report;
int ps_debug_poison(uint32_t index_word, uint64_t value_word, ps_poison_report* report, int32_t cap, int32_t* n_report);

/* ---- kernel-level test hooks (K1/K2 matrices vs oracle dumps) ----
 * Runs Alignment::update (cpp/Alignment.cpp:63-73) for one event on the current sequence
 * and returns the dense (n_levels+1) x (n_states+1) forward or backward main matrix with
 * out-of-band cells as NaN; direction 0 = forward (column index = ref position), 1 = backward
 * (column index k = -col, cpp/Alignment.cpp:284-285).  stay (may be NULL) gets the stay matrix.
 * Step codes are returned for the forward matrix only — the only ones the reference ever reads
 * (backtrace, cpp/Alignment.cpp:516-624); for direction 1 they are zero. */
int ps_debug_fill(ps_align* a, int32_t ev, int32_t direction, double* main, double* stay,
                  uint8_t* step_main, uint8_t* step_stay);
/* The forward log tables of ps_posterior_stats for one event, as k_post_fwd left them: main = M and stay = S (may be NULL), dense
 * (n_levels+1) x (n_states+1), NaN outside the band, 0 in the blank column and in the columns without a state, -infinity for S on a
 * band's first row; shaped like ps_debug_fill's.  An inert event has the blank column only.  The checkers do not export it. */
int ps_debug_posterior(ps_align* a, int32_t ev, double* main, double* stay);
/* The tables of ViterbiMutate (cpp/Viterbi.cpp:239-426) for n AlignData, run as ps_batch_viterbi_mutate runs them (same launches,
 * deviates from the calling thread's generator).  obs_build selects the emission kernel: 0 = the library's choice, 1 = k_vit_obs_lds
 * (at most 72 events), 2 = k_vit_obs<64> (at most 64), 3 = k_vit_obs<256>; PS_ERR_BAD_ARG for a build that cannot take the batch's
 * event count (the checkers have one emission loop and ignore it).  Outputs, region r at a row pitch of cap_T (PS_ERR_BAD_ARG when a
 * region keeps more positions; T is written first): T[n] positions kept; obs[n][cap_T][1024] trimmed-mean emissions;
 * bp[n][cap_T][1024] back-pointers; lik_final[n][1024]; fwd[n][cap_T][1024] forward vectors as the recursion left them, each row up
 * to its own scale (nkeep > 0 only); paths[n][max(nkeep, 1)][cap_T] the STATE paths (nkeep = 0: the one deterministic back-trace).
 * Any output but T may be NULL.  The reference shim has no such view: PS_ERR_UNSUPPORTED. */
int ps_debug_viterbi(int32_t n, ps_align* const* a, int32_t obs_build, int32_t nkeep, double skip_prob, double stay_prob,
                     double mut_min, double mut_max, int64_t cap_T, int32_t* T, double* obs, int16_t* bp, double* lik_final,
                     double* fwd, int16_t* paths);
/* The recursion and the back-traces alone, on emission rows and deviates from the caller (no AlignData): n_regions regions of T[r]
 * rows, concatenated.  obs[sum T][1024]; deviates (nkeep > 0): per region a [nkeep][T[r]] block in the order the traces consume
 * them (trace k, last position first), region r's block at nkeep * (T[0] + .. + T[r-1]); trace k runs at the attenuation
 * mut_min + (mut_max - mut_min) k / nkeep.  Outputs bp[sum T][1024], lik_final[n_regions][1024], fwd[sum T][1024] (nkeep > 0),
 * paths laid out like the deviates with max(nkeep, 1) traces; any may be NULL.  The HIP library skips only its emission kernel
 * (exp(obs) is formed on the host) and launches k_vit_steps / k_vit_log / k_vit_trace as a production call does. */
int ps_debug_viterbi_steps(int32_t n_regions, const int32_t* T, const double* obs, const double* deviates, int32_t nkeep,
                           double skip_prob, double stay_prob, double mut_min, double mut_max, int16_t* bp, double* lik_final,
                           double* fwd, int16_t* paths);

/* Tuning knob (process-wide): forward-only alignment batches — ScoreAlignments, FindMutations' candidate sequences — of at
 * least `min_alignments` jobs run as strip sweeps (ps_sweep.hip / ps_sweepw.hip: one to four wavefronts per alignment, ps_set_sweep_form);
 * smaller ones a workgroup per alignment (k_fill),
 * which finishes a lone small batch sooner.  Results do not depend on it.  Negative: back to the default
 * (PORESEQ_SWEEP_MIN, else 400). */
int ps_set_sweep_min(int32_t min_alignments);
/* The same for Alignment::update batches (ScoreMutations: a forward and a backward sweep per alignment, with score matrices):
 * from `min_sweeps` sweeps on, strip sweeps with full records.  Negative: the default (PORESEQ_SWEEP2_MIN, else never:
 * their records cap a launch at a few hundred sweeps, where a workgroup per sweep is twice as fast — DESIGN.md section 4). */
int ps_set_sweep2_min(int32_t min_sweeps);
/* Alignment::update batches whose edit lists read at most a quarter of the matrix columns (every ScoreMutations call of a consensus
 * schedule except Refine's point edits at every position): from `min_sweeps` sweeps on, strip sweeps that store the
 * {main, stay} records of the columns scoreMutation / columnMax will read (cpp/Alignment.cpp:447-512, cpp/Alignment.h:181-214) and
 * nothing else of the score matrices.  Negative: the default (PORESEQ_SPARSE_MIN, else 160).  Results do not depend on it. */
int ps_set_sparse_min(int32_t min_sweeps);
/* The form every strip sweep tries first: `rows_per_lane` rows of the band per lane on `wavefronts` (1, 2 or 4) wavefronts per
 * (alignment, direction) — ps_sweep.hip / ps_sweepw.hip; a band too wide for it takes the next larger form.  rows_per_lane <= 0 with
 * wavefronts 1 / 2 / 4: that many wavefronts, the smallest strip height whose band fits; both <= 0: the library's own choice (by
 * launch size; PORESEQ_SWEEP_FORM=K,NW).  Returns PS_ERR_BAD_ARG for a form that is not built.
 * Results do not depend on it (the reference has one serial loop per alignment, cpp/Alignment.cpp:83-99). */
int ps_set_sweep_form(int32_t rows_per_lane, int32_t wavefronts);
/* The part of the device's memory THIS PROCESS plans for (process-wide; default 1, or PORESEQ_DEVICE_FRACTION): the slabs for full
 * score matrices, every runtime's share and the ceiling of the device pools are fractions of it.  One process per GPU leaves it
 * alone; ranks that share a GPU set 1 / (ranks on the device) before their first compute call (poreseq_amd.dist.init does).
 * fraction <= 0 restores the default; > 1 is PS_ERR_BAD_ARG.  Not part of the reference's interface (its processes share nothing). */
int ps_set_device_fraction(double fraction);

/* Hot-kernel instrumentation for bench.py: accumulated HIP-event time (ms), launches and
 * algorithmic bytes of the named kernel class ("fill" = k_fill, "sweep" = the strip sweeps k_sweep / k_sweeps / k_sweep2 and their _w builds,
 * "score", "viterbi", "sw", "point_table" = k_point_table: 8 bytes per (event, edit) read, 88 per position written, "support" = k_support: 8 bytes per (event, edit) read, 8 + 24 n_groups per edit written, "genotype" = k_genotype: 8 per (event, edit) read, 8 (n_frac + 1) + 4 per edit written,
 * "link" = k_link: 8 per (event, edit) read, 32 window per edit written, "phase" = k_phase: 32 window per edit read, 16 per edit written,
 * "haptag" = k_haptag: 8 per (event, edit) and 16 per edit read, 24 max_sets per event written,
 * "align_stats" = k_align_stats: 16 per level read, 112 per event written,
 * "kmer_stats" = k_kmer_stats: 24 per level read, 48 * 1024 * n_groups per region written,
 * "move_stats" = k_move_stats: 8 per level read, 64 per event and, with the per-level arrays, 5 per level written) since reset; host-side launch counts by form under "sweep_w2", "sweep_w4", "sweep_kept", "sw_pk8", "slab",
 * "fill_pair" / "fill_pair_fwd" / "fill_cmp" / "fill_512" / "fill_1024" / "fill_wide" (which form a k_fill launch took), "score_g7" .. "score_g64"
 * (k_score's size classes) and "fill_ieee" / "sweep_ieee" / "score_ieee" (launches that took the IEEE-division build);
 * Smith-Waterman batches by traceback form under "sw_lists", "sw_summary", "sw_map"; "remap" = k_remap launches and "variant_chunks" =
 * alignment chunks (launches) over distinct sequences (units) of ps_score_sequences; "likes_dev" / "likes_host" = chunks of FindMutations'
 * candidate sequences whose per-base likelihood vectors came from k_likes / from the host loop (a sequence of more than 12 284 states in
 * the chunk, or PORESEQ_DEBUG_LIKES_HOST=1). */
/* ps_prof_enable(1) makes every hot-kernel launch be bracketed by HIP events on the library's stream
 * (one extra synchronisation per launch: use it in a separate, untimed pass); ps_prof_enable(2) queues the
 * event pairs instead and reads them when the profile is asked for (no synchronisation per launch: usable
 * inside a timed region).  The profile belongs to the calling thread's runtime.  ps_prof_reset zeroes the sums. */
int ps_prof_enable(int32_t on);
int ps_prof_reset(void);
int ps_prof_get(const char* name, double* ms, int64_t* launches, double* alg_bytes);
/* work units of the class since reset: "fill" / "sweep" = sweeps (one alignment, one direction), "score" = (event, edit) items */
int ps_prof_units(const char* name, double* units);

#ifdef __cplusplus
}
#endif
#endif /* PORESEQ_HIP_H_ */
