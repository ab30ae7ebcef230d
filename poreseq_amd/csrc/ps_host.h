// ps_host.h — host-side structures of libporeseq_hip.so
#ifndef PS_HOST_H_
#define PS_HOST_H_

#include <functional>

#include "ps_internal.h"
#include "ps_ownplan.h"   // OwnKind and the output plan of the own-sequence statistics (host-only, no HIP)

namespace ps {

const char* last_error();

// PORESEQ_TRACE=1: wall-clock phase timers on stderr (host-side tuning aid)
struct Tick {
    const char* what; double t0; bool on;
    explicit Tick(const char* w);
    void lap(const char* label);
};

struct Align;

void rand_seed(unsigned seed);   // per-thread generator of ViterbiMutate's deviates (ps_vit.cpp)
int rand_next();
struct RandState;                // an explicit generator state (one per region of a lock-step driver)
RandState* rand_state_new(unsigned seed);
void rand_state_free(RandState* r);
void rand_state_seed(RandState* r, unsigned seed);
int rand_state_next(RandState* r);   // nullptr: the calling thread's generator

struct JobSpec {
    Align* a = nullptr;                                  // owner of the event data (one batch may mix several AlignData)
    int ev = 0;
    const std::vector<int>* states = nullptr;
    double *ra = nullptr, *rl = nullptr, *ri = nullptr;  // device arrays of the job
    JobOut* out = nullptr;                               // device result record of the job
    // column-sparse Alignment::update (ScoreMutations with a short edit list): per direction the device table of kept-column
    // indices (C + 2 entries, -1: not kept) and the number of kept columns
    const int* keep[2] = {nullptr, nullptr};
    int nkeep[2] = {0, 0};
};

// a set of alignment jobs with all their device workspaces carved out of the runtime pool
struct Batch {
    std::vector<JobD> jobs;
    BatchD d;
    int ndir = 1, P = 0, Pmax = 64, maxC = 0, maxn = 0, maxlbn = 0;
    int64_t maxS = 0, cells = 0, ncols = 0;
    // strip sweeps (forward-only batches, ps_sweep.hip)
    std::vector<SweepJob> sjobs;
    SweepD sd;
    int sweep_K = 0, sweep_NW = 1, sweep_maxT = 0;
    int64_t sweep_code_bytes = 0, sweep_sb = 0, sweep_recs = 0;
    bool sparse = false;          // ndir == 2: records of the kept columns only (JobSpec.keep)
    char* ext = nullptr;          // full matrices go here (a slab) instead of the runtime's own pools
    size_t ext_bytes = 0;
    std::vector<int> nkeep;       // [2 * job + direction]
    MoveRun moves;                // forward-only batches: k_move_stats behind the walk (ps_move_stats); unset: today's chain
    int build(Runtime* rt, const std::vector<JobSpec>& specs, int ndir, int lb_extra);
    int place(Runtime* rt, int P, bool can_split = false);
    double fill_alg_bytes() const;
};

// AlignData (cpp/AlignData.h:26-35) with the event data resident in HBM
struct Align {
    std::string bases;
    std::vector<int> states;
    ps_params par = {4.5, 150, 300, 0};  // cpp/AlignUtil.h:64
    int E = 0;
    std::vector<int> n;
    std::vector<int64_t> off;
    int64_t ntot = 0;
    std::vector<std::string> evseqs;
    std::vector<double> h_mean, h_stdv, h_ra, h_rl, h_model, h_trans;   // h_trans: log transition probabilities [E][4]
    bool host_refs_valid = true;
    void* slab = nullptr;
    size_t slab_cap = 0;
    void* last_stream = nullptr;   // the stream that last had work on the slab enqueued (hipStream_t; Batch::build, create, refs_to_host): align_slab_give
    double *d_mean = nullptr, *d_stdv = nullptr, *d_lsd = nullptr, *d_ra = nullptr, *d_rl = nullptr, *d_ri = nullptr;
    double *d_model = nullptr, *d_trans = nullptr;
    double *d_model8 = nullptr, *d_lev[2] = {nullptr, nullptr};   // k_fill's tables (ps_internal.h, JobD)
    std::string nonfinite;                                        // first level / model row whose emissions are -infinity or NaN (ps_sane.h); empty: none
    bool fastdiv = true;                                          // tabulated reciprocals are usable (all divisors sane)
    JobOut* d_out = nullptr;
    std::map<std::string, std::vector<double>> seqlikes;  // cpp/AlignData.h:34

    ~Align();
    int create(Runtime* rt, const char* seq, int64_t seq_len, int32_t n_events, const int64_t* level_off,
               const double* mean, const double* stdv, const double* ref_align, const double* ref_like,
               const double* model, const double* trans, const char* evseq, const int64_t* evseq_off,
               const ps_params* params);
    JobSpec job(int e);   // event e against this AlignData's own sequence
    // event e against another sequence: its states, reference arrays of all events of this AlignData (laid out like the slab's), its result record
    JobSpec job(int e, const std::vector<int>* other, double* ra, double* rl, double* ri, JobOut* out);
    int base_batch(Runtime* rt, Batch* b, int ndir, int lb_extra);   // job(e) of every event
    int refs_to_host(Runtime* rt);
    int refs_to_host_async(Runtime* rt);   // enqueue; refs_finish() after the stream has been synchronised
    void refs_finish();
    double *pend_ra = nullptr, *pend_rl = nullptr;
    // ref_align / ref_like as the last call that writes back left them (ps_align_keep_refs): a call that only scores realigns the
    // events as a side effect, and the reference drops that realignment with its scratch AlignData
    double* d_keep = nullptr;      // [2][ntot], allocated by the first keep_refs()
    bool keep_valid = false;       // d_keep holds the refs of the last write-back point; make_mutations (a call that writes back) clears it
    bool restore_due = false;      // a scoring call was announced since: the refs may have left d_keep
    int keep_refs(Runtime* rt);    // remember the current refs, unless d_keep already holds them
    int restore_refs(Runtime* rt); // back to the kept refs (ref_index and the spans with them), if a scoring call may have moved them
};

void accumulate_likes(const double* ra, const double* rl, int n, int C, double* likes);

// strip sweeps (ps_sweep.hip, ps_sweepw.hip): K rows per lane on NW wavefronts per sweep
// The forms that are built, X(K, on one wavefront, on two, on four) by ascending K: the one list that the form search, the sweep
// launchers of both files and the backtrace launcher are made from (PS_FORM_1(code): code, PS_FORM_0(code): nothing)
#define PS_SWEEP_HEIGHTS(X) \
    X(2, 0, 0, 1) X(3, 0, 0, 1) X(4, 1, 1, 1) X(5, 0, 1, 0) X(6, 1, 1, 1) X(10, 1, 1, 0) X(16, 1, 0, 0) X(24, 1, 0, 0) X(32, 1, 0, 0)
#define PS_FORM_1(...) __VA_ARGS__
#define PS_FORM_0(...)
struct SweepForm { int K = 0, NW = 1; bool ok() const { return K > 0; } };
int sweep_guess_k(int W);                         // strip height of the one-wavefront form for realign_width W (0: too wide for a strip sweep)
int sweep_guess_window(int W, int K);             // strips in band on one step, probably, at realign_width W
SweepForm sweep_guess_form(int W, int NW);        // form to try first on NW wavefronts (K = 0: none)
SweepForm sweep_next_form(SweepForm f, int win);  // next larger one after a window of `win` strips did not fit (K = 0: none)
bool sweep_form_exists(int K, int NW);
int sweep_win_max(int NW);                        // widest window of strips a sweep on NW wavefronts supports
double sweep_job_bytes(int n0, int C, SweepForm f, bool full = false);   // bytes of one job: step codes (+ both directions' records)
int sweep_prepare(Runtime* rt, Batch& b, SweepForm f);  // band / qlo tables + the widest window (b.sd.maxwin, device)
void sweep_form_set(int K, int NW);               // tests / tuning: the form every strip sweep tries first (K <= 0: the library's choice)
int sweep_run(Runtime* rt, Batch& b);             // sweeps, maxima, backtrace, path scores (b.sd.codes placed by the caller)
void sweep_min_set(int n);                        // forward-only batches of at least n alignments take the strip sweep (< 0: default)
void sweep2_min_set(int n);                       // the same for Alignment::update batches (sweeps = 2 per alignment)
void sparse_min_set(int n);                       // Alignment::update batches whose edit list reads few columns: strip sweeps with kept columns from n sweeps on
int sparse_min();                                 // that threshold as it stands (the default when none was set)
int launch_likes(Runtime* rt, const BatchD& b, const LikeGroup* d_groups, int ngroups, double* d_out);   // per-base likelihood vectors on the device
int likes_max_states();                           // longest sequence (states) k_likes takes
bool sweep_enabled();                             // PORESEQ_NO_SWEEP unset
double fwd_job_bytes(const Align* a, int n0, int C);   // device bytes one forward-only alignment job will probably take

constexpr int PS_SPLIT = 1;   // realign(): the matrices would exceed `cap` bytes; nothing was launched, b.P holds the width they need
int realign(Runtime* rt, Batch& b, double cap = 0.0);
// the *_multi forms run the same call for several AlignData (independent regions) in one launch chain
void par_for(int n, const std::function<void(int)>& fn);
int find_mutations_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<std::string>*>& seeds,
                         const std::vector<std::vector<Mut>*>& outs);
// Every event of an AlignData aligned forward-only to a sequence that is not its own, for any number of such (AlignData, sequence)
// units, in as many launch chains (chunks) as this runtime's share of the device allows (ps_fwd.cpp): FindMutations' seeds,
// ps_score_sequences.  The driver cuts the chunks, sizes and carves "seed_refs" and "seed_out", builds the jobs, runs updaterefs and
// realign, and cuts a chunk again whose bands came out wider than guessed; the two callbacks are what the callers differ in.
struct FwdUnit { Align* a; const std::vector<int>* states; };   // the events of `a` against this sequence
struct FwdChunk {                      // what a callback sees of the chunk being run
    size_t q0 = 0, q1 = 0, nref = 0, njobs = 0;   // units [q0, q1), their levels, their jobs (unit by unit, event by event)
    std::vector<size_t> roff;          // level offset of unit q - q0 in the chunk's arrays (event e of it: + a->off[e])
    double *d_ra = nullptr, *d_rl = nullptr, *d_ri = nullptr;   // [nref] each: ref_align, ref_like, ref_index of the chunk's jobs
    Batch b;                           // (collect) after the fills
};
typedef std::function<int(FwdChunk&)> FwdStep;
// place: put ref_align of the chunk's jobs into d_ra and clear d_rl, enqueued on rt->stream (staging taken here is released with the
// chunk).  collect: after realign; read what the caller wants and return with the stream idle.  what: "seed" / "variant", for the
// trace.  tk: laps "seed batch build" before the fills.  *nchunks: chunks that ran to the end.
int fwd_chunks(Runtime* rt, const std::vector<FwdUnit>& units, const char* what, const FwdStep& place, const FwdStep& collect,
               int* nchunks = nullptr, Tick* tk = nullptr);
int gather_best(Runtime* rt, const Batch& b, double** best);   // the jobs' maxima through "best": *best[job] is readable once the stream has been synchronised
// Variant.py:48-61 (`variant -v`) for several AlignData: scores[r][s * E + e] = ScoreEvents()[e] of a copy of as[r] realigned to seqs[r][s],
// accuracy[r][s] = swalign's identity in % (may be nullptr); no AlignData is modified (ps_variant.hip)
int score_sequences_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<std::string>*>& seqs,
                          const std::vector<double*>& scores, const std::vector<double*>& accuracy);
std::string info_string();   // process-wide state in one line (ps_info)
struct MemInfo { size_t slabs = 0, slab_bytes = 0; int slabs_planned = 0; long long pool_bytes = 0; };
MemInfo mem_info();          // ps_mem.cpp's part of it: slabs allocated (and their bytes) of how many, bytes in the pools of this process
void for_idle_runtimes(const std::function<void(Runtime&)>& fn);   // fn on every runtime no thread owns, under the free list's lock
int hwq_mode(std::string* why);   // 1: every stream on one priority level (a hardware queue each), 0: streams dealt over the levels, 2: a private queue per stream within a budget, the rest dealt
int peak_runtimes();   // most host threads that ever owned a runtime at the same time
int live_runtimes();   // host threads that currently own a runtime
int guess_slots(const Align* a);   // anti-diagonal footprint realign() will probably choose
// A lock-step call over n AlignData that may not fit the device in one piece re-issues itself over sub-ranges, sub(k0, k1), one after
// the other: the fewest sub-batches of about equal size that fit (share_cut, ps_plan.h), when AlignData k probably takes need(k) of
// share_cap(ndir) bytes — or two halves, when the bands came out wider than guessed
double share_need(const Align* a, int ndir);   // device bytes the events of `a` will probably take at `ndir` sweeps each
double share_cap(int ndir);                    // this runtime's device share; for full forward + backward matrices (ndir == 2) what a slab holds
template <class Need> bool over_share(size_t n, int ndir, Need&& need) { return share_cut(0, n, share_cap(ndir), need) < n; }
template <class Need, class Sub> int in_share_chunks(size_t n, int ndir, Need&& need, Sub&& sub) {
    for (size_t k0 = 0; k0 < n;) {
        const size_t k1 = share_cut(k0, n, share_cap(ndir), need);
        PS_TRY(sub(k0, k1));
        k0 = k1;
    }
    return PS_OK;
}
template <class Sub> int in_halves(size_t n, Sub&& sub) {
    PS_TRY(sub(0, n / 2));
    return sub(n / 2, n);
}
void device_fraction_set(double f);   // the part of the device this process plans for (several ranks on one GPU); <= 0: PORESEQ_DEVICE_FRACTION, else 1
double device_fraction();
double device_share_bytes();   // this runtime's share of the device memory for its own pools (step codes, kept columns, small matrices)
// a process-wide slab for the full score matrices of one Refine-sized ScoreMutations call (ps_mem.cpp)
struct SlabHold { void* s = nullptr; char* p = nullptr; size_t bytes = 0; hipStream_t drain = nullptr; void release(); ~SlabHold() { release(); } };   // release() drains `drain` first: nothing in flight may still use the slab
int slab_acquire(SlabHold* h);    // blocks while all slabs are taken
size_t slab_bytes();
double dense_cap_bytes();         // bytes of full matrices one call may place
// the matrix pools of a batch ("rec", "flg"): carved out of the slab the batch holds (bt.ext), else the runtime's own, re-sized
int ensure_matrix_pools(Runtime* rt, const Batch& bt, size_t need_rec, size_t need_flg, bool can_split, void** rec_out, void** flg_out);
int align_slab_take(Runtime* rt, size_t bytes, void** out, size_t* cap);   // an AlignData's slab, from the process-wide cache when one fits
void align_slab_give(void* slab, size_t cap, void* last_stream);           // and back to it (or freed)
int make_mutations_multi(Runtime* rt, const std::vector<Align*>& as, std::vector<std::vector<Mut>> muts, std::vector<int>* nbases);
// One AlignData of an edit-scoring call (ps_score.cpp): its handle, its edit list and, of the outputs below, those the call's EditKind
// means — host arrays, null where the caller does not want one; score_edits checks the ranges and the required ones.  A lock-step call is an array of these; a sub-batch (a call cut to
// fit the share, or halved because its bands came out wider than guessed) is a sub-range of the same array.
struct EditReq {
    Align* a = nullptr;
    const std::vector<Mut>* muts = nullptr;   // the list to score (Points: FindPointMutations', made by score_edits into `own`)
    // List: the scored copy of the list, and [E][M] every event's term of every edit's score (optional)
    std::vector<Mut>* out = nullptr; double* delta = nullptr;
    // Points: [states][9] rows and [states] per-position records (either may be null), the position count the caller sized them for
    double* table = nullptr; ps_point_best* best = nullptr; int64_t npos_given = 0;
    // Support, Genotype: [E] group ids below ngroups, [M] scores (optional), [M][ngroups] records (Genotype: optional)
    const int32_t* group = nullptr; int ngroups = 0; double* score = nullptr; ps_edit_support* rec = nullptr;
    // Genotype: [nfrac] alt fractions, [M][nfrac + 1] likelihoods, [M] covering-event counts (optional)
    int nfrac = 0; const double* frac = nullptr; double* lik = nullptr; int32_t* ncover = nullptr;
    // Phase: window, vote threshold and tagged sets, [M] scores (`score`, optional), [M][window] links, [M]
    // phase records, [E][max_sets] event records (optional), the number of sets (optional)
    int window = 0; double min_link = 0.0; int max_sets = 0;
    ps_edit_link* link = nullptr; ps_edit_phase* phase = nullptr; ps_event_hap* hap = nullptr; int32_t* nsets = nullptr;
    // filled by score_edits: the plan, the list of a Points call and its point_layout
    EditPlan plan;
    std::vector<Mut> own;
    std::vector<int> pos_first, pos_triv;
};
// ScoreMutations (cpp/MakeMutations.cpp:23-69) and its reductions for reqs[0 .. n - 1] in one launch chain (rt: null for a reduction,
// whose runtime is taken once its arguments are checked and there is an edit to score)
int score_edits(Runtime* rt, EditKind kind, EditReq* reqs, size_t n);
// One AlignData of a call that aligns every event to the AlignData's own sequence, forward only (ps_own.cpp): its handle and, of the
// host outputs below, those the call's OwnKind means.  A lock-step call is an array of these, a sub-batch a sub-range of it.
struct OwnReq {
    Align* a = nullptr;
    double* scores = nullptr;          // [E] the events' scores after a realignment (Score: required; the statistics: optional)
    double* likes = nullptr;           // Score: [bases] the per-base likelihoods of all events, added up (optional)
    ps_event_stats* stats = nullptr;   // AlignStats: [E] records
    // KmerStats: [E] group ids below ngroups, [ngroups][NS] cells, written in full
    const int32_t* group = nullptr; int ngroups = 0; ps_kmer_cell* table = nullptr;
    // MoveStats: [E] records; [E] pointers to [n_e] step codes / columns each (either may be null, and so may an entry)
    ps_event_moves* moves = nullptr; uint8_t* const* step = nullptr; int32_t* const* col = nullptr;
    // Posterior: [E] records; [E] pointers to [n_e] doubles each, both or neither (an entry may be null for an event without levels)
    ps_event_posterior* post = nullptr; double* const* emit = nullptr; double* const* pcol = nullptr;
};
// ScoreAlignments (cpp/MakeMutations.cpp:148-195) | ps_batch_align_stats: per event the census of ref_align and the sums of the
// scaling fit | ps_batch_kmer_stats: per AlignData, event group and 5-mer state the sums of a model re-estimation | ps_batch_move_stats:
// per event the backtrace's moves, counted between the walk and the kernel that overwrites its records (ps_stats.hip) |
// ps_batch_posterior_stats: per event the sum over all alignments in its band and the expected moves under it (ps_post.hip) — the
// band stage of the fills, k_post_fwd, k_post_bwd; no backtrace, the handles' refs stay what they are (`realign` is ignored): enum
// class OwnKind { Score, AlignStats, KmerStats, MoveStats, Posterior }, ps_ownplan.h.  reqs[0 .. n - 1] in one launch chain.  realign:
// ScoreAlignments' fills and backtraces first (Score, MoveStats: always); without, the statistics reduce the refs the handles hold
int own_forward(Runtime* rt, OwnKind kind, bool realign, OwnReq* reqs, size_t n);
int score_mutations(Runtime* rt, Align* a, const std::vector<Mut>& muts, std::vector<Mut>* out);
void find_point_mutations(const Align* a, std::vector<Mut>* out);
int make_mutations(Runtime* rt, Align* a, std::vector<Mut> muts, int* nbases);
int find_mutations(Runtime* rt, Align* a, const std::vector<std::string>& seeds, std::vector<Mut>* out);
// One ViterbiMutate call (ps_vit.cpp): its arguments, the entry point and whether a refusal names a region index (a lock-step
// call), and the table tap of the test hooks (ps_internal.h), null in production
struct VitCall {
    int nkeep = 0;
    double skip = 0.0, stay = 0.0, mmin = 0.0, mmax = 0.0;
    const char* who = "ps_batch_viterbi_mutate";
    bool lockstep = true;
    VitTap* tap = nullptr;
};
// and one AlignData of it: its handle, its generator (null: the calling thread's) and where its sequences go.  A lock-step call is an
// array of these.
struct VitReq {
    Align* a = nullptr;
    RandState* rng = nullptr;
    std::vector<std::string>* out = nullptr;
};
// ViterbiMutate (cpp/Viterbi.cpp:239-426) for reqs[0 .. n - 1] in as few launch chains as the share allows (rt: null, the runtime is
// taken once the arguments are checked)
int viterbi_mutate(Runtime* rt, const VitCall& call, VitReq* reqs, size_t n);
// one sub-batch of it on the device: regs[0 .. n - 1] through emissions, steps and back-traces into their `paths`
int viterbi_batch(Runtime* rt, const VitCall& call, VitRegionH* regs, size_t n);
int debug_fill(Runtime* rt, Align* a, int ev, int dir, double* main, double* stay, uint8_t* sm, uint8_t* ss);
// ps_debug_posterior (ps_own.cpp): the chain of a Posterior call for one event, its forward tables un-skewed
int debug_posterior(Runtime* rt, Align* a, int ev, double* main, double* stay);
// ps_debug_poison (ps_mem.cpp): overwrites the scratch memory the calling thread's next call could find left over (ps_poison.h)
int debug_poison(Runtime* rt, uint32_t index_word, uint64_t value_word, ps_poison_report* rep, int32_t cap, int32_t* n_rep);
// ps_debug_viterbi / ps_debug_viterbi_steps (include/poreseq_hip.h): the tables of a ViterbiMutate call
int debug_viterbi(const std::vector<Align*>& as, int build, int nkeep, double skip, double stay, double mmin, double mmax,
                  int64_t cap_T, int32_t* T, double* obs, int16_t* bp, double* lik_final, double* fwd, int16_t* paths);
int debug_viterbi_steps(Runtime* rt, int R, const int32_t* T, const double* obs, const double* rnd, int nkeep, double skip, double stay,
                        double mmin, double mmax, int16_t* bp, double* lik_final, double* fwd, int16_t* paths);

}  // namespace ps
#endif
