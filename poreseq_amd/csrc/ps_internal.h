// ps_internal.h — shared declarations of libporeseq_hip.so (host side + kernel launchers).
//
// Data layout in HBM:
//   levels      mean/stdv/logstdv f64, all events concatenated               (read-only per PSAlign call)
//   models      per event 6 x 1024 f64: lev_mean, lev_stdv, log_lev, sd_mean, sd_lambda, log_lambda
//   refs        per alignment job ref_align / ref_like / ref_index f64[n0]   (rewritten by the backtrace)
//   DP matrices per (job, direction): "skewed" storage  REC[s][slot], s = i + j (anti-diagonal),
//               slot = i mod P, one 16-byte record {main, stay} per cell, plus (forward) FLG[s][slot] u16
//               = {main step, stay step, score <= 0 bits}.  One anti-diagonal is one contiguous run of
//               P records: the fill kernel's stores are fully coalesced.
#ifndef PS_INTERNAL_H_
#define PS_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/poreseq_hip.h"
#include "ps_greedy.h" // struct Mut, apply_edit, greedy_apply (host-only, no HIP)
#include "ps_editplan.h" // NS, states_of, EditPlan, PT_SLOTS, SCORE_CLASSES and the size classes of k_score (host-only, no HIP)
#include "ps_plan.h"   // MAT_FRONT, MAT_BACK and the memory plan's arithmetic (host-only, no HIP)

namespace ps {

constexpr double BIG = 1e300;  // "inf" of the reference, cpp/AlignUtil.h:20

// ---- error plumbing ------------------------------------------------------------------------
int fail(int code, const std::string& msg);
bool trace_on();   // PORESEQ_TRACE is set (read once): diagnostics on stderr
#define PS_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return ps::fail(PS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)
#define PS_LAUNCH_CHECK() PS_HIP(hipGetLastError())
#define PS_TRY(expr)            \
    do {                        \
        int _rc = (expr);       \
        if (_rc != PS_OK) return _rc; \
    } while (0)

// ---- runtime: device, stream, grow-only device buffers -------------------------------------
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);  // grow-only; contents are NOT preserved across growth
    hipError_t release();      // frees and forgets the buffer and takes it off the process's pool count, whatever hipFree answers (returned)
    template <class T> T* as() const { return (T*)p; }
};

// grow-only pinned host buffer (hipHostMalloc): device->host copies into it are truly asynchronous
struct HBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    template <class T> T* as() const { return (T*)p; }
};

// Pinned staging arena: host<->device copies of per-call tables go through it so that hipMemcpyAsync is a
// plain enqueue (a pageable source makes the runtime stage the copy itself and block the calling thread, which
// also serialises concurrent host threads).  Memory handed out stays valid until reset(); the arena is reset at
// the next API entry of the owning thread, after its streams have drained.
struct Stage {
    struct Chunk { char* p; size_t cap; };
    std::vector<Chunk> chunks;
    size_t used = 0;          // bytes used in the last chunk
    bool dirty = false;
    void* alloc(size_t bytes);   // 256-byte aligned, nullptr when pinned memory cannot be had
    int reset();
    // scoped reuse inside one API call: everything allocated after mark() is handed back by release(); the caller
    // guarantees that no copy touching that memory is still in flight
    size_t mark() const { return chunks.size() <= 1 ? used : (size_t)-1; }
    void release(size_t m) { if (m != (size_t)-1 && chunks.size() <= 1) used = m; }
};

struct Prof { double ms = 0; int64_t launches = 0; double bytes = 0; double units = 0; };

struct Runtime {
    bool ready = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;          // Smith-Waterman batches run here, concurrently with the alignment fills
    hipEvent_t ev0 = nullptr, ev1 = nullptr, sw0 = nullptr, sw1 = nullptr;
    std::map<std::string, DBuf> pool;
    std::map<std::string, HBuf> hpool;
    HBuf& hbuf(const std::string& name) { return hpool[name]; }
    std::map<std::string, Prof> prof;
    bool prof_on = false;
    // prof_defer: event pairs are queued and read when the profile is asked for (ps_prof_get) instead of after every launch, so
    // that profiling does not serialise the host with the stream (bench.py profiles inside its timed region this way)
    bool prof_defer = false;
    struct ProfPend { hipEvent_t a, b; const char* name; double bytes; };
    std::vector<ProfPend> prof_pend;
    std::vector<hipEvent_t> prof_spare;
    DBuf& buf(const std::string& name) { return pool[name]; }
    Stage stage;
    // enqueue host -> device through the arena (the source may die as soon as this returns)
    int up(void* dst, const void* src, size_t bytes, hipStream_t st = nullptr);
    // enqueue device -> host into arena memory; *hptr is readable after the stream has been synchronised
    int down(void** hptr, const void* src, size_t bytes, hipStream_t st = nullptr);
    template <class T> int down(T** hptr, const void* src, size_t count) { return down((void**)hptr, src, count * sizeof(T)); }
};
int runtime(Runtime** out);  // PS_ERR_NO_DEVICE when no usable GPU; never falls back
// The stream Smith-Waterman batches should use: the runtime's second stream (created on first use), so that the batch overlaps with
// the base realign of FindMutations — while the calling thread is the only one inside the library.  With several threads (lock-step
// batches in flight) every runtime keeps to one stream: HIP maps streams onto 4 hardware queues by default (ps_runtime.cpp).
int second_stream(Runtime* rt, hipStream_t* out);
int live_runtimes();   // host threads that currently own a runtime (ps_runtime.cpp)

// ---- mutation list: struct Mut, with Sequence(original, mut) and the greedy pass of MakeMutations, in ps_greedy.h (no HIP) ----

// ---- device-side job descriptor: one (event, sequence) alignment ---------------------------
// Everything a kernel needs about a job hangs off the descriptor itself (device pointers into the owning
// AlignData's slab), so one batch can mix jobs of several AlignData handles (regions refined in lock-step).
struct JobOut;
struct JobD {
    const double* model8; // derived model of the job's event per 5-mer, rows of MODEL_ROW_BYTES: mean, 1/stdv, stdv, log stdv, sd mean, 1/sd mean, lambda, log lambda (k_fill)
    const double* lev[2]; // level records per direction, [n0][4]: forward row i -> {mean[i-1], stdv[i-1], 3 lsd[n0-i], 1/stdv[i-1]},
                          //                                      backward row i -> the same of level n0-i (cpp/Alignment.cpp:171-172, 345-349)
    const int* st;        // 5-mer states of the job's sequence [C] (4 ints of -1 padding on either side)
    double lsk, lst, lex, lin;   // log transition probabilities: skip, stay, extend, insert
    double lik_offset;
    int n0;          // levels in the event
    int C;           // states of the job's sequence
    int W;           // realign_width (band half-width of the fills)
    int force_inert; // realign_width == 0: every Alignment is a no-op (cpp/Alignment.cpp:85-86)
    int P;           // slots per anti-diagonal (multiple of 64, >= widest footprint + 9; k_fill_wide: multiple of 128, >= footprint + 2)
    int lbn;         // entries in each lb table (C + 2 + extra)
    int K;           // 0: skewed matrices (k_fill); > 0: strip matrices of K rows per lane (k_sweep2): REC[step][row of the strip][lane];
                     // < 0: column-sparse records (k_sweeps): only the columns an edit list reads, REC[kept column][row - band start]
    int pitch;       // column-sparse records: records per kept column (>= rows of the widest band)
    int NL;          // strip matrices: lanes of a sweep (64 per wavefront of its workgroup); strip q sits on lane q mod NL
    const int* keep[2];  // column-sparse records: per direction, kept-column index of column j (0 .. C + 1) or -1
    int64_t lb_off;      // lb table the fills were made with          (int32[lbn])
    int64_t lbn_off;     // lb table after the latest backtrace        (int32[lbn])
    int64_t mat_off[2];  // record offset of anti-diagonal 0 of the forward / backward matrix
    int64_t lo_off[2];   // into LO / HI (int32 per anti-diagonal)
    int64_t col_off[2];  // into per-column arrays (C+1 entries per direction)
    int64_t S;           // anti-diagonals: n0 + C + 1
    double* ra;          // ref_align  [n0]
    double* rl;          // ref_like   [n0]
    double* ri;          // ref_index  [n0]
    JobOut* out;         // per job results (persist in the AlignData between calls for its own events)
};

// per job results living in device memory
struct JobOut {
    double best;      // forward maxScore.score after the last column
    int bi, bj;       // its cell
    int has_index;    // ref_index non-empty after the latest updaterefs
    int refstart, refend;
    int inert;        // latched at the start of an API call: the reference's stripe_width == 0
    int term_i, term_w;   // where the latest backtrace stopped (bt_walk, ps_dev.h): row; column << 3 | matrix << 2 | kind
};

constexpr int MODEL_ROW_BYTES = 80;   // k_fill's model rows: 8 doubles + 16 bytes of padding (LDS bank spread)
constexpr int LO_PAD = 160;    // LO / HI entries behind S, all -1 (k_fill prefetches them in chunks of 64)

struct SweepJob;
// device pointers of the pools a batch of jobs lives in (filled by Batch::build / place)
struct BatchD {
    const JobD* jobs;
    int njobs;
    int* lb;                              // pool of lb tables
    int* lo;                              // lowest in-band row per anti-diagonal (-1: none)
    int* hi;                              // highest in-band row per anti-diagonal
    double2* rec;                         // matrices {main, stay}, skewed
    unsigned short* flg;                  // forward matrices: step words {main step, stay step << 8, score <= 0 bits}
    double* cmax;                         // per column max of main
    double* pm;                           // prefix max over columns (MaxInfo.score per column)
    int* maxw;                            // widest band footprint of any job of the batch on one anti-diagonal (sizes P)
    int fastdiv;                          // every AlignData of the batch allows k_fill's tabulated reciprocals
    double log2pi;
    // strip matrices (JobD.K > 0, k_sweep2): the sweep jobs (2 per job: forward, backward) and their band / qlo / qhi tables
    const SweepJob* s_sj;
    const int2* s_band;
    const int* s_qlo;
    const int* s_qhi;
};

// ---- strip sweeps (ps_sweep.hip): forward-only alignments, one wave per job ------------------------
struct StripBest;
struct SweepJob {           // per job, parallel to BatchD.jobs
    int64_t codes_off;      // bytes into the code pool: step t of the job starts at codes_off + t * NL * K
    int64_t band_off;       // into band (int2 {i0, i1} per column, C + 2 entries)
    int64_t q_off;          // into qlo (int per step, T + 8 entries)
    int64_t sb_off;         // into the per-strip maxima (Q entries)
    int T;                  // steps: t = column + strip runs 1 .. T - 1
    int Q;                  // strips of K rows
};
struct SweepD {
    const SweepJob* sj;
    int2* band;
    int* qlo;
    int* qhi;               // lowest / highest strip in band per step (-1: none)
    unsigned char* codes;   // one byte of storage per cell, seven raw predicate bits of the fill (ps_codes.h: CB_*, code_fetch)
    StripBest* sb;
    int* maxwin;            // widest window of strips in band on one step, over the batch
    int K;
    int nl;                 // lanes of a sweep: 64 per wavefront (ps_sweepw.hip: two or four wavefronts per sweep)
    int ndir;               // 1: forward-only jobs; 2: sweep job jd = 2 * job + direction
    int sparse;             // ndir == 2: records of the kept columns only (JobD.keep) instead of every cell's
};

// one sequence's jobs (its events, in order) for the per-base likelihood vector of ScoreAlignments (k_likes, ps_sweep.hip)
struct LikeGroup {
    int job0, njobs;        // the sequence's jobs inside the batch
    int C, len;             // states of the sequence; doubles of its vector (bases)
    int64_t out_off;        // into the output pool
};

// the runtime BatchD.fastdiv as a kernel's template argument: launch(std::true_type / std::false_type)
template <class F> void with_fastdiv(int fastdiv, F&& launch) { if (fastdiv) launch(std::true_type()); else launch(std::false_type()); }

// ---- kernel launchers (ps_kernels.hip; launch_score: ps_edit.hip) ------------------------------------------------------
int launch_updaterefs(Runtime* rt, const BatchD& b);
int launch_lb(Runtime* rt, const BatchD& b, int which /*0: lb_off, 1: lbn_off*/, int maxlbn);
int launch_lo(Runtime* rt, const BatchD& b, int ndir, int64_t maxS);
int launch_fill(Runtime* rt, const BatchD& b, const std::vector<JobD>& jobs, int ndir, int64_t maxS, int P, int64_t ncols);
struct MoveRun;
int launch_backtrace(Runtime* rt, const BatchD& b, int maxn, const MoveRun& moves);   // moves: k_move_stats between the walk and k_fill_like, when asked for
int launch_prefix(Runtime* rt, const BatchD& b, int ndir);

struct ScoreArgs {
    int job0, njobs;           // the AlignData's jobs inside the batch
    int nitems_per_job;        // M
    int ncolmax;               // max new columns of any edit
    int ws;                    // scoring_width
    const int* m_start;        // [M]
    const int* m_mlen;         // [M] len(mut)
    const int* m_cm;           // [M] states of the edited sequence
    const int* m_ncol;         // [M] new columns actually produced
    const int* m_skip;         // [M] 1: edit skipped (start > len)
    const int* m_states;       // [M][ncolmax] states of the new columns
    const int* m_oldidx;       // [M] index into the unique-r0 list
    const int* r0;             // [nr0] unique max(start-3,1) values
    int nr0;
    double* old;               // [njobs][nr0]
    double* oldall;            // NULL, or [njobs][oldall_pitch]: column-pair maxima of every column (k_oldall), when the list touches most columns
    int64_t oldall_pitch, maxS;
    double* delta;             // [njobs][M]
    double* score;             // [M]
    // device lists of edit indices by new-column count (score_class, ps_editplan.h)
    const int* cls_items[SCORE_CLASSES];
    int cls_count[SCORE_CLASSES];
};
// A point-edit table call (k_point_table instead of k_reduce) has one of these per AlignData beside its ScoreArgs — a record of its
// own, so that ScoreArgs and with it the device code of every other scoring kernel stay what they were.  The list is
// FindPointMutations' and position p's edits are pos_first[p] .. pos_first[p + 1] - 1 (8 of them for an A / C / G / T base, 9 for
// any other character).
struct PointArgs {
    const int* pos_first;      // [npos + 1]
    const int* pos_triv;       // [npos] slot 1 .. 4 of the trivial substitution (the position's own base), 0: none
    int npos;                  // positions with a row: states of the sequence (0: nothing to write for this AlignData)
    double* table;             // NULL, or [npos][9]
    ps_point_best* best;       // NULL, or [npos]
};
// A support call (k_support instead of k_reduce, ps_score_mutation_support) likewise has one of these per AlignData beside its
// ScoreArgs: the events' group ids and where the scores and the per-(edit, group) records go.
struct SupportArgs {
    const int* group;          // [njobs] group id of every event, 0 .. ngroups - 1
    int ngroups;               // 1 .. SUPPORT_MAX_GROUPS (0: nothing to write for this AlignData)
    double* score;             // [M]
    ps_edit_support* out;      // [M][ngroups]
};
constexpr int SUPPORT_MAX_GROUPS = 8;
// A genotype call (ps_score_mutation_genotypes: k_genotype behind k_support) has one of these per AlignData beside its ScoreArgs and
// SupportArgs: the alt fractions f and g = 1 - f, and where the likelihoods and the covering-event counts go.  `score` is set for
// an AlignData whose caller wants no support records (its SupportArgs.ngroups is 0 and k_support leaves at once): k_genotype then
// writes the score, k_reduce's sum, itself.
constexpr int GENO_MAX_FRAC = 8;
struct GenoArgs {
    int nfrac;                 // 0 .. GENO_MAX_FRAC (-1: nothing to write for this AlignData)
    double f[GENO_MAX_FRAC], g[GENO_MAX_FRAC];
    double* score;             // NULL, or [M]
    double* lik;               // [M][nfrac + 1]
    int* ncover;               // [M]
};
// A phase call (ps_score_mutation_phase: k_link, k_phase and k_haptag behind k_score) has one of these per AlignData beside its
// ScoreArgs: the window, the vote threshold, the number of tagged sets and where the records go.  `score`, `hap` and `nsets` are
// null where the caller does not want them.
constexpr int LINK_MAX_WINDOW = 8;
constexpr int PHASE_MAX_SETS = 8;
struct PhaseArgs {
    int W;                     // 1 .. LINK_MAX_WINDOW (0: nothing to write for this AlignData)
    int S;                     // 1 .. PHASE_MAX_SETS
    double min_link;
    double* score;             // NULL, or [M]
    ps_edit_link* link;        // [M][W]
    ps_edit_phase* phase;      // [M]
    ps_event_hap* hap;         // NULL, or [njobs][S]
    int* nsets;                // one
};
// What an edit-scoring call makes of k_score's [event][edit] matrix: a scored list (ScoreMutations), rows per position (ps_point_table),
// scores and per-group records (ps_score_mutation_support), those with genotype likelihoods behind them, or pair links, phase
// sets and read haplotypes (ps_score_mutation_phase)
enum class EditKind { List, Points, Support, Genotype, Phase };
// One such call as launch_score runs it: the descriptors of its AlignData on the host (`pts` for Points, `sps` for Support and
// Genotype, `gts` for Genotype, `phs` for Phase; the others stay empty) and where their copies lie on the device (null where the
// vector is empty)
struct ScoreLaunch {
    EditKind kind = EditKind::List;
    std::vector<ScoreArgs> sas; std::vector<PointArgs> pts; std::vector<SupportArgs> sps; std::vector<GenoArgs> gts; std::vector<PhaseArgs> phs;
    const ScoreArgs* d_sas = nullptr; const PointArgs* d_pts = nullptr; const SupportArgs* d_sps = nullptr; const GenoArgs* d_gts = nullptr;
    const PhaseArgs* d_phs = nullptr;
};
int launch_score(Runtime* rt, const BatchD& b, const ScoreLaunch& L);
int launch_begin(Runtime* rt, const BatchD& b);
int launch_gather_best(Runtime* rt, const BatchD& b, double* out);   // out[job] = the job's forward maxScore (JobOut.best)

// Alignment census and the sums of the scaling fit (ps_stats.hip, ps_align_stats): one event as k_align_stats sees it, and one
// AlignData's events inside the call's list of them
struct StatJob {
    const double* ra;     // ref_align [n]
    const double* mean;   // level means [n]
    const double* model;  // the event's model, rows of NS: level_mean, level_stdv (the first two of d_model's six)
    const int* st;        // 5-mer states of the sequence [S]
    int n, S;
    const double* stdv;   // level stdvs [n] (k_kmer_stats)
    int grp, pad;         // the event's group (k_kmer_stats; 0 for k_align_stats)
};
struct StatRegion { int job0, njobs, ngroups, tab0; };   // ngroups, tab0: the region's groups and its first table row (k_kmer_stats)
// grid (maxE, nregs): out[job] for every job of every region; alg_bytes for the profile ("align_stats")
int launch_align_stats(Runtime* rt, const StatJob* d_jobs, const StatRegion* d_regs, int nregs, int maxE, double alg_bytes, ps_event_stats* d_out);
// Per-k-mer model statistics (ps_stats.hip, ps_kmer_stats): grid (KMER_BLOCKS x maxG, nregs); d_out[(tab0 + g) * NS + k] for every
// group g of every region; alg_bytes for the profile ("kmer_stats")
constexpr int KMER_TILE = 512;     // levels staged in LDS per step
constexpr int KMER_BLOCKS = 4;     // workgroups per (region, group): 256 k-mers each
int launch_kmer_stats(Runtime* rt, const StatJob* d_jobs, const StatRegion* d_regs, int nregs, int maxG, double alg_bytes, ps_kmer_cell* d_out);
// The backtrace's moves (ps_stats.hip, ps_move_stats): one event as k_move_stats sees it — the walk's records in ref_like's slot
// (bt_walk, ps_dev.h), where the walk started and stopped, and where the per-level arrays go (null: not asked for)
struct MoveJob {
    const long long* rec;   // [n] column << 4 | step code << 1 | matrix of every recorded level, 0 elsewhere
    const JobOut* out;      // bi / bj, term_i / term_w, inert
    uint8_t* step;          // NULL, or [n]
    int32_t* col;           // NULL, or [n]
    int n, pad;
};
// A batch's request for k_move_stats, on the host-side Batch: the kernel runs between the walk and the first kernel that
// overwrites the walk's records, with arguments of its own (BatchD and JobD stay what they are).  jobs == nullptr: not asked for.
struct MoveRun {
    const MoveJob* jobs = nullptr;        // device, one per job of the batch, in job order
    const StatRegion* regs = nullptr;     // device, one per AlignData (job0, njobs)
    int nregs = 0, maxE = 0;
    ps_event_moves* out = nullptr;        // device, [jobs]
    double alg_bytes = 0.0;
};
// grid (maxE, nregs): out[job] for every job of every region; counted in the profile as "move_stats".  No-op without a request.
int launch_move_stats(Runtime* rt, const MoveRun& mv);

// Posterior move counts (ps_post.hip, ps_posterior_stats): where one event's per-level arrays go (both null: not asked for), and its
// per-row sums: scratch of the two kernels, reduced in row order so that no result depends on the slots per anti-diagonal
struct PostJob {
    double* emit;   // NULL, or [n]
    double* col;    // NULL, or [n]
    double* row;    // [n][8]
};
constexpr int POST_MAX_SLOTS = 1024;   // slots per anti-diagonal of the posterior kernels: one lane each, one workgroup per event
// k_post_fwd, then k_post_bwd, one workgroup of P threads per job of the batch (its skewed records placed, JobD.P = P, a multiple of
// 64 up to POST_MAX_SLOTS): out[job] in full; counted in the profile as "post_fwd" / "post_bwd", `cells` band cells for its bytes
int launch_post(Runtime* rt, const BatchD& b, int P, const PostJob* d_jobs, ps_event_posterior* d_out, double cells);

// Smith-Waterman (kernels: ps_sw.hip, host side: ps_swhost.cpp)
int sw_device(Runtime* rt, const std::string& s1, const std::string& s2, int* score, double* accuracy,
              std::vector<int>* inds1, std::vector<int>* inds2);
void sw_band_counters(int64_t out[5]);   // band mode: pairs banded, fell back, maxima near a band edge, band cells, full-matrix cells

// Viterbi (kernels and launchers: ps_viterbi.hip, the chain: ps_vit.cpp).  One region (AlignData) of a sub-batch as the kernels see it
struct VitReg {
    const double* model;   // [E][6][1024]
    int E, T;              // events, reference positions kept
    int64_t in_off;        // into obsin (doubles)
    int64_t t_off;         // first position of the region in obs / eobs / bp / lfwd (rows of 1024)
};
// and on the host: what the chain reads of it and where its paths go.  A call is one array of these, a sub-batch a sub-range of it.
struct VitRegionH {
    int E = 0, T = 0;
    int index = -1;                      // of the region in the caller's lock-step batch, named in a refusal (-1: not a batch)
    const double* obsin = nullptr;       // [T][E][4]: level, sd, log sd, present
    const double* d_model = nullptr;     // device, [E][6][1024]
    void* rng = nullptr;                 // the region's generator state, handed to draw()
    void (*draw)(void* rng, double* out /*[nkeep][T]*/, size_t n) = nullptr;
    std::vector<int16_t> paths;          // out: [max(nkeep, 1)][T] states; empty for a region without positions
};
// Table tap of viterbi_batch for the test hooks ps_debug_viterbi / ps_debug_viterbi_steps (ps_debug.cpp): a null pointer in
// production.  The same launches, grids and buffers run whether it is set or not; with a tap the tables are also copied to the
// host.  Results are appended (viterbi_mutate may cut a batch into several sub-batches), regions in batch order.
struct VitTap {
    int obs_build = 0;                  // in: emission build: 0 the library's choice, 1 k_vit_obs_lds, 2 k_vit_obs<64>, 3 k_vit_obs<256>
    const double* obs_rows = nullptr;   // in: [sum T][1024] emission rows from the caller; the emission kernel is skipped, exp(obs) is formed on the host
    std::vector<int> T;                 // per region
    std::vector<double> obs;            // [sum T][1024]
    std::vector<short> bp;              // [sum T][1024]
    std::vector<double> lik_final;      // [regions][1024]
    std::vector<double> fwd;            // [sum T][1024] as k_vit_steps wrote it, before k_vit_log (nkeep > 0 only: no forward table otherwise)
    std::vector<std::vector<int16_t>> paths;   // per region [nkeep or 1][T] states, as VitRegionH.paths
};
bool vit_obs_lds_ok();   // k_vit_obs_lds can have its dynamic LDS (asked once per process)
// emission build 1 k_vit_obs_lds | 2 k_vit_obs<64> | 3 k_vit_obs<256> over ttot positions (counted in the profile as vit_obs_lds / vit_obs_64 / vit_obs_256)
void launch_vit_obs(Runtime* rt, int build, const VitReg* d_regs, const int* d_posreg, const double* d_in, int64_t ttot, int maxE, double* d_obs, double* d_eobs);
int launch_vit_steps(Runtime* rt, const VitReg* d_regs, int R, const double* d_obs, const double* d_eobs, double skip, double stay, short* d_bp, double* d_fwd,
                     double* d_lik, bool keep_fwd);
// k_vit_log over the forward table, then k_vit_trace: nkeep back-traces per region
int launch_vit_trace(Runtime* rt, const VitReg* d_regs, int R, int64_t ttot, int nkeep, double* d_fwd, const int* d_start, double skip, double stay,
                     const double* d_att, const double* d_rnd, short* d_path);

void prof_flush(Runtime* rt);   // deferred mode: read the queued event pairs (drains the stream)
void prof_begin(Runtime* rt);
void prof_end(Runtime* rt, const char* name, double alg_bytes);

}  // namespace ps

#endif
