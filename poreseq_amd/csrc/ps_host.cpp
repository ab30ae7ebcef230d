// ps_host.cpp — host side of libporeseq_hip.so above the runtime: alignment batches (Batch::build / place), realign() (which fill
// runs for a batch, in which form), what a lock-step call may take of the device (guess_slots, share_need, share_cap), and
// MakeMutations (cpp/MakeMutations.cpp).  struct Align — AlignData — is in ps_align.cpp; ScoreAlignments and the two statistics
// calls, one chain over the events' own sequences, in ps_own.cpp; ScoreMutations and its reductions — the edit-scoring chain — in
// ps_score.cpp, the edit plans in ps_editplan.h, FindMutations in ps_find.cpp, ViterbiMutate's host chain in ps_vit.cpp.  The runtime, its streams and par_for
// are in ps_runtime.cpp; device memory — pools, shares, slabs, the AlignData slab cache — in ps_mem.cpp, its arithmetic in ps_plan.h.
// All dynamic-programming arithmetic runs in the HIP kernels (ps_kernels.hip, ps_edit.hip, ps_sw.hip,
// ps_viterbi.hip); there is no CPU implementation of it in this library.
#include "ps_host.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace ps {

// ------------------------------------------------------------------------------------------ batch
int Batch::build(Runtime* rt, const std::vector<JobSpec>& specs, int ndir_, int lb_extra) {
    ndir = ndir_;
    P = 0; Pmax = 64;
    d.fastdiv = 1;
    jobs.clear();
    maxS = 0; maxC = 0; maxn = 0; maxlbn = 0;
    sparse = ndir == 2 && !specs.empty();
    nkeep.clear();
    constexpr int ST_PAD = 8;   // ints of -1 around every state list: k_fill fetches four states per 16-byte load
    int64_t st_tot = 0, lb_tot = 0, lo_tot = 0, col_tot = 0;
    std::vector<int> h_states;
    std::map<const std::vector<int>*, int64_t> st_seen;
    std::vector<int64_t> st_at(specs.size());
    for (size_t k = 0; k < specs.size(); k++) {
        const JobSpec& s = specs[k];
        const Align* a = s.a;
        s.a->last_stream = (void*)rt->stream;   // (every kernel over an AlignData's events goes through a Batch: ~Align, slab cache)
        const int W = a->par.realign_width;
        if (W < 0) return fail(PS_ERR_BAD_ARG, "realign_width < 0");
        // widest possible footprint 2W + 1, plus the idle slots k_fill wants between two rows of a lane; the slots actually
        // used follow the measured footprint (realign), typically (2W + 1) / (1 + levels per base) + 9
        const int pm = std::max(64, ((2 * W + 10 + 63) / 64) * 64);
        Pmax = std::max(Pmax, std::min(pm, 2048));
        JobD j;
        memset(&j, 0, sizeof(j));
        j.model8 = a->d_model8 + (size_t)s.ev * (MODEL_ROW_BYTES / 8) * NS;
        j.lev[0] = a->d_lev[0] + 4 * a->off[s.ev]; j.lev[1] = a->d_lev[1] + 4 * a->off[s.ev];
        if (!a->fastdiv) d.fastdiv = 0;
        j.lsk = a->h_trans[s.ev * 4 + 0]; j.lst = a->h_trans[s.ev * 4 + 1]; j.lex = a->h_trans[s.ev * 4 + 2]; j.lin = a->h_trans[s.ev * 4 + 3];
        j.lik_offset = a->par.lik_offset;
        j.n0 = a->n[s.ev]; j.C = (int)s.states->size(); j.W = W; j.P = 0;
        j.force_inert = (W == 0) ? 1 : 0;
        j.lbn = j.C + 2 + lb_extra;
        auto it = st_seen.find(s.states);
        if (it == st_seen.end()) {
            h_states.insert(h_states.end(), ST_PAD, -1);
            st_seen[s.states] = st_tot + ST_PAD; st_at[k] = st_tot + ST_PAD;
            h_states.insert(h_states.end(), s.states->begin(), s.states->end());
            h_states.insert(h_states.end(), ST_PAD, -1);
            st_tot += j.C + 2 * ST_PAD;
        } else st_at[k] = it->second;
        j.lb_off = lb_tot; lb_tot += j.lbn;
        j.lbn_off = lb_tot; lb_tot += j.lbn;
        j.S = (int64_t)j.n0 + j.C + 1;
        for (int d = 0; d < ndir; d++) {
            j.lo_off[d] = lo_tot; lo_tot += j.S + LO_PAD;
            j.col_off[d] = col_tot; col_tot += j.C + 1;
        }
        j.ra = s.ra; j.rl = s.rl; j.ri = s.ri; j.out = s.out;
        j.keep[0] = s.keep[0]; j.keep[1] = s.keep[1];
        if (!s.keep[0] || !s.keep[1]) sparse = false;
        nkeep.push_back(s.nkeep[0]); nkeep.push_back(s.nkeep[1]);
        maxS = std::max(maxS, j.S); maxC = std::max(maxC, j.C); maxn = std::max(maxn, j.n0); maxlbn = std::max(maxlbn, j.lbn);
        jobs.push_back(j);
    }
    ncols = col_tot;
    PS_TRY(rt->buf("jobs").ensure(std::max<size_t>(jobs.size(), 1) * sizeof(JobD)));
    PS_TRY(rt->buf("states").ensure(std::max<size_t>(h_states.size(), 1) * sizeof(int)));
    PS_TRY(rt->buf("lb").ensure(std::max<int64_t>(lb_tot, 1) * sizeof(int)));
    PS_TRY(rt->buf("lo").ensure(std::max<int64_t>(lo_tot, 1) * sizeof(int)));
    PS_TRY(rt->buf("hi").ensure(std::max<int64_t>(lo_tot, 1) * sizeof(int)));
    PS_TRY(rt->buf("cmax").ensure(std::max<int64_t>(col_tot, 1) * sizeof(double)));
    PS_TRY(rt->buf("pm").ensure(std::max<int64_t>(col_tot, 1) * sizeof(double)));
    PS_TRY(rt->buf("maxw").ensure(64));
    const int* d_states = rt->buf("states").as<int>();
    for (size_t k = 0; k < jobs.size(); k++) jobs[k].st = d_states + st_at[k];
    PS_TRY(rt->up(rt->buf("jobs").p, jobs.data(), jobs.size() * sizeof(JobD)));
    PS_TRY(rt->up(rt->buf("states").p, h_states.data(), h_states.size() * sizeof(int)));
    d.jobs = rt->buf("jobs").as<JobD>();
    d.njobs = (int)jobs.size();
    d.lb = rt->buf("lb").as<int>(); d.lo = rt->buf("lo").as<int>(); d.hi = rt->buf("hi").as<int>();
    d.rec = nullptr; d.flg = nullptr;
    d.s_sj = nullptr; d.s_band = nullptr; d.s_qlo = nullptr; d.s_qhi = nullptr;
    d.cmax = rt->buf("cmax").as<double>(); d.pm = rt->buf("pm").as<double>();
    d.maxw = rt->buf("maxw").as<int>();
    d.log2pi = std::log(2 * M_PI);  // cpp/AlignUtil.h:24
    return PS_OK;
}

// second phase: the anti-diagonal footprint of every band is known, size the skewed matrices
int Batch::place(Runtime* rt, int P_, bool can_split) {
    P = std::min(Pmax, std::max(64, ((P_ + 63) / 64) * 64));
    if (const char* fp = getenv("PORESEQ_DEBUG_MIN_P")) P = std::min(1024, std::max(P, (atoi(fp) + 63) / 64 * 64));  // tests / experiments: more slots than needed
    int64_t mat_tot = 0;
    for (JobD& j : jobs) {
        j.P = P;
        // spare anti-diagonals in front of and behind every matrix: k_fill's pipeline starts early and runs past S
        for (int dd = 0; dd < ndir; dd++) { j.mat_off[dd] = mat_tot + (int64_t)MAT_FRONT * P; mat_tot += matrix_cells(j.S, P); }
    }
    cells = mat_tot;
    void *prec = nullptr, *pflg = nullptr;
    PS_TRY(ensure_matrix_pools(rt, *this, (size_t)std::max<int64_t>(mat_tot, 1) * sizeof(double2), (size_t)std::max<int64_t>(mat_tot, 1) * sizeof(unsigned short), can_split, &prec, &pflg));
    PS_TRY(rt->up(rt->buf("jobs").p, jobs.data(), jobs.size() * sizeof(JobD)));
    d.rec = (double2*)prec; d.flg = (unsigned short*)pflg;
    return PS_OK;
}

// bytes the fills of this batch move by the SURVEY 8(d) accounting: 18 B (fwd) / 16 B (back) per band cell
double Batch::fill_alg_bytes() const {
    double t = 0;
    for (const JobD& j : jobs) {
        const double band = std::min<double>(2.0 * j.W + 1, j.n0);
        t += (double)j.C * band * (ndir == 2 ? 34.0 : 18.0) + 24.0 * j.n0 * ndir;
    }
    return t;
}

// ------------------------------------------------------------------------------------------ realign
// forward fill + backtrace + updaterefs of a batch (the body of ScoreAlignments per event,
// cpp/MakeMutations.cpp:148-195, and of Alignment::update with ndir == 2, cpp/Alignment.cpp:63-73)
static int sweep_min_default() { static const int v = getenv("PORESEQ_SWEEP_MIN") ? atoi(getenv("PORESEQ_SWEEP_MIN")) : 400; return v; }
static int sweep2_min_default() { static const int v = getenv("PORESEQ_SWEEP2_MIN") ? atoi(getenv("PORESEQ_SWEEP2_MIN")) : (1 << 30); return v; }
// column-sparse Alignment::update (ScoreMutations whose edit list reads few columns): from this many sweeps on.  A wave per sweep
// takes ~27 ms for a 10 kb event whatever the chip could do, a workgroup per sweep ~11-14 ms: a lone driver thread's small batches
// (one region: 20 sweeps) finish sooner on k_fill.  With several lock-step batches in flight the chip is shared and what counts is
// the SIMD time a sweep holds (1.6x less as a wave) and the CUs it leaves to the other batches: every size takes the sweep.
static int sparse_min_default() {
    static const int v = getenv("PORESEQ_SPARSE_MIN") ? atoi(getenv("PORESEQ_SPARSE_MIN")) : -1;
    return v >= 0 ? v : (live_runtimes() > 1 ? 0 : 160);
}
static std::atomic<int> g_sweep_min(-1), g_sweep2_min(-1), g_sparse_min(-1);
void sweep_min_set(int n) { g_sweep_min.store(n); }
void sweep2_min_set(int n) { g_sweep2_min.store(n); }
void sparse_min_set(int n) { g_sparse_min.store(n); }
int sparse_min() { return g_sparse_min.load() >= 0 ? g_sparse_min.load() : sparse_min_default(); }
bool sweep_enabled() { static const bool off = getenv("PORESEQ_NO_SWEEP") != nullptr; return !off; }

// PORESEQ_DEBUG_SWEEP_K (tests: a given strip height, i.e. a wrong guess; read per call); < 0: not set
static int debug_sweep_k() { const char* e = getenv("PORESEQ_DEBUG_SWEEP_K"); return e ? std::max(atoi(e), 0) : -1; }

// device bytes one forward-only job of AlignData a (n0 levels against C states) will probably take: step codes of a strip sweep,
// or the skewed {record, step word} matrix of k_fill
double fwd_job_bytes(const Align* a, int n0, int C) {
    SweepForm f;
    if (sweep_enabled()) f = sweep_guess_form(a->par.realign_width, 1);
    if (f.ok() && debug_sweep_k() > 0) f.K = debug_sweep_k();
    if (f.ok()) return 1.15 * sweep_job_bytes(n0, C, f);   // (the multi-wavefront forms take up to a tenth more: more steps, fewer rows per lane)
    return matrix_bytes((int64_t)n0 + C + 1, guess_slots(a), 1);
}

// Which form a strip-sweep launch takes (ps_sweep.hip: K rows per lane on NW wavefronts per sweep).  Forced by
// ps_set_sweep_form / PORESEQ_SWEEP_FORM=K,NW (tests, tuning); else by the launch's size: a wavefront alone on its SIMD issues one
// vector instruction per ~5 cycles whatever the chip could do, so a launch that cannot fill the chip's SIMDs with one wavefront per
// sweep spreads every sweep over two or four.
static std::atomic<int> g_form_K(0), g_form_NW(0);
void sweep_form_set(int K, int NW) { g_form_K.store(K); g_form_NW.store(NW); }
static SweepForm pick_form(int W, int nsweeps, bool fastdiv) {
    SweepForm f;
    int fk = g_form_K.load(), fnw = g_form_NW.load();
    if (fk <= 0 && fnw <= 0) {                                    // (the API has precedence: the environment speaks only when neither was set)
        static const char* e = getenv("PORESEQ_SWEEP_FORM");
        if (e && sscanf(e, "%d,%d", &fk, &fnw) != 2) { fk = 0; fnw = 0; }
    }
    if (fk > 0 && sweep_form_exists(fk, fnw) && (fnw == 1 || fastdiv)) { f.K = fk; f.NW = fnw; return f; }
    if (fk <= 0 && (fnw == 1 || fnw == 2 || fnw == 4)) {         // only the wavefronts per sweep are given: the smallest strip height that fits
        for (int nw = fastdiv ? fnw : 1; nw >= 1; nw >>= 1) { f = sweep_guess_form(W, nw); if (f.ok()) return f; }
        return f;
    }
    // Two wavefronts per sweep by default: the SIMD time of one (K = 10) in half the time and three wavefronts per SIMD instead of two
    // (measured: 2 400 sweeps of 10 kb in 50 ms against 58; 20 in 13 ms against 23).  Four — a quarter more SIMD time, 11 ms — only for
    // a lone driver thread's small launches: with several lock-step batches in flight the chip is shared and SIMD time is what counts.
    constexpr int W4_MAX = 256;   // sweeps per launch up to which four wavefronts each pay
    int nw = live_runtimes() <= 1 && nsweeps <= W4_MAX ? 4 : 2;
    if (!fastdiv) nw = 1;                                         // (the multi-wavefront builds exist with tabulated reciprocals only)
    for (; nw >= 1; nw >>= 1) {
        f = sweep_guess_form(W, nw);
        // a narrow band on many wavefronts leaves most lanes without a strip: at least half of them busy, else fewer wavefronts
        if (f.ok() && (nw == 1 || sweep_guess_window(W, f.K) * 2 >= 64 * nw)) return f;
    }
    return sweep_guess_form(W, 1);
}

// Strip sweeps (ps_sweep.hip): one to four wavefronts per alignment and direction.  Forward-only batches (ScoreAlignments) keep one
// byte per cell; Alignment::update batches (ndir == 2, ScoreMutations) also the {main, stay} records of both directions, in strip
// order or of the kept columns only.  Returns -1 when the batch has to take the k_fill path instead (band too wide for any form).
static int realign_sweep(Runtime* rt, Batch& b, double cap) {
    int W = 0;
    for (const JobD& j : b.jobs) W = std::max(W, j.W);
    SweepForm f = pick_form(W, b.d.njobs * b.ndir, b.d.fastdiv != 0);
    if (const int dbg = debug_sweep_k(); dbg >= 0) { f.K = dbg; f.NW = 1; }   // tests: a given strip height first
    if (!f.ok()) return -1;
    PS_TRY(launch_begin(rt, b.d));
    PS_TRY(launch_lb(rt, b.d, 0, b.maxlbn));
    for (;;) {
        PS_TRY(sweep_prepare(rt, b, f));
        int* w = nullptr;
        PS_TRY(rt->down(&w, b.sd.maxwin, (size_t)1));
        PS_HIP(hipStreamSynchronize(rt->stream));
        { if (trace_on()) fprintf(stderr, "[ps] realign (strip sweep%s): %d jobs x %d, K = %d on %d wavefronts, widest window %d strips\n", b.sparse ? ", kept columns" : "", b.d.njobs, b.ndir, f.K, f.NW, *w); }
        if (*w <= sweep_win_max(f.NW)) break;
        f = sweep_next_form(f, *w);
        if (!f.ok()) { for (JobD& j : b.jobs) j.K = 0; return -1; }
    }
    const int K = f.K;
    const double bytes = (double)b.sweep_code_bytes + 16.0 * (double)b.sweep_recs;
    if (cap > 0 && bytes > cap) {
        if (trace_on()) fprintf(stderr, "[ps] realign (strip sweep): %.2f GB of step codes%s at K = %d, over the share: split\n", bytes * 1e-9, b.ndir == 2 ? (b.sparse ? " and kept columns" : " and records") : "", K);
        b.P = 0;
        return PS_SPLIT;
    }
    {
        // forward-only: the step codes live in the pool of the score matrices (a runtime runs one batch at a time: never both);
        // with both directions the records take that pool and the codes the step words'
        const size_t need_rec = b.ndir == 2 ? (size_t)std::max<int64_t>(b.sweep_recs, 1) * sizeof(double2) : (size_t)std::max<int64_t>(b.sweep_code_bytes, 1);
        const size_t need_flg = b.ndir == 2 ? (size_t)std::max<int64_t>(b.sweep_code_bytes, 1) : 0;
        void *prec = nullptr, *pflg = nullptr;
        Batch own;   // (kept columns and step codes are small: always the runtime's own pools)
        const int rc = ensure_matrix_pools(rt, b.sparse || b.ndir == 1 ? own : b, need_rec, need_flg, cap > 0, &prec, &pflg);
        if (rc == PS_ERR_NOMEM && cap > 0) { b.P = 0; return PS_SPLIT; }
        PS_TRY(rc);
        b.sd.codes = b.ndir == 2 ? (unsigned char*)pflg : (unsigned char*)prec;
        if (b.ndir == 2) {
            b.d.rec = (double2*)prec; b.d.flg = nullptr;
            b.d.s_sj = b.sd.sj; b.d.s_band = b.sd.band; b.d.s_qlo = b.sd.qlo; b.d.s_qhi = b.sd.qhi;
            PS_TRY(rt->up(rt->buf("jobs").p, b.jobs.data(), b.jobs.size() * sizeof(JobD)));   // JobD.K, JobD.mat_off
            PS_HIP(hipMemsetAsync(b.d.cmax, 0, b.ncols * sizeof(double), rt->stream));
        }
    }
    if (rt->prof_on) { rt->prof["sweep"].bytes += b.fill_alg_bytes(); rt->prof["sweep"].units += (double)b.d.njobs * b.ndir; }
    PS_TRY(sweep_run(rt, b));
    PS_TRY(launch_updaterefs(rt, b.d));
    return PS_OK;
}

int realign(Runtime* rt, Batch& b, double cap) {
    if (!b.d.njobs) return PS_OK;
    // forward-only batches take the strip sweep (one wave per alignment) from ps_set_sweep_min / PORESEQ_SWEEP_MIN alignments on
    // (default 400); a smaller batch alone on the chip finishes sooner with a workgroup per alignment (k_fill: ~11 ms against
    // ~25 ms for a 10 kb sweep; with several batches in flight the two take the same time)
    if (b.sparse && !(sweep_enabled() && b.d.njobs * 2 >= sparse_min())) b.sparse = false;
    const int sweep_min = b.ndir == 1 ? (g_sweep_min.load() >= 0 ? g_sweep_min.load() : sweep_min_default())
                                      : (b.sparse ? 0 : (g_sweep2_min.load() >= 0 ? g_sweep2_min.load() : sweep2_min_default()));
    // (a forward-only batch below the threshold whose skewed matrices would not fit this runtime's share — a third of FindMutations'
    //  candidate batches with many batches in flight — takes the sweep as well: 7 MB of step codes per alignment instead of 140 MB)
    bool too_big = false;
    if (b.ndir == 1 && sweep_enabled() && b.d.njobs < sweep_min) {
        double est = 0;
        for (const JobD& j : b.jobs) est += matrix_bytes(j.S, guess_slots_w(j.W), 1);   // (not guess_slots: the tests' override of the guess does not reach here)
        too_big = est > device_share_bytes();
    }
    if (sweep_enabled() && (b.d.njobs * b.ndir >= sweep_min || too_big)) {
        const int rc = realign_sweep(rt, b, cap);
        if (rc != -1) return rc;
    }
    b.sparse = false;   // (a band too wide for any strip height: skewed matrices)
    PS_TRY(launch_begin(rt, b.d));
    PS_TRY(launch_lb(rt, b.d, 0, b.maxlbn));
    PS_TRY(launch_lo(rt, b.d, b.ndir, b.maxS));
    int* w = nullptr;
    PS_TRY(rt->down(&w, b.d.maxw, (size_t)1));
    PS_HIP(hipStreamSynchronize(rt->stream));
    // nine slots more than the widest footprint: a lane idles at least nine anti-diagonals between two rows, so a prefetch
    // window of k_fill (fetched six steps ahead, four steps long) never spans two rows of a lane that has a cell
    // (a footprint beyond 1015 rows takes k_fill_wide: two slots per thread, up to 2048 slots, P a multiple of 128)
    if (std::max(*w, 1) + 2 > 2048)
        return fail(PS_ERR_UNSUPPORTED, "band footprint of " + std::to_string(*w) + " rows on one anti-diagonal: wider than two slots per lane of one "
                                        "workgroup (2046); realign_width up to 1022 fits for any input");
    { if (trace_on()) fprintf(stderr, "[ps] realign: %d jobs x %d, widest footprint %d\n", b.d.njobs, b.ndir, *w); }
    const int Pneed = std::max(*w, 1) + 9 <= 1024 ? std::max(*w, 1) + 9 : ((std::max(*w, 1) + 2 + 127) / 128) * 128;
    if (cap > 0) {   // the caller sized this batch on a guess of the footprint: let it split when the real one is much wider
        const int Pr = std::min(b.Pmax, std::max(64, ((Pneed + 63) / 64) * 64));
        double bytes = 0;
        for (const JobD& j : b.jobs) bytes += matrix_bytes(j.S, Pr, b.ndir);
        if (bytes > cap) {
            if (trace_on()) fprintf(stderr, "[ps] realign: %.1f GB of matrices at %d slots per anti-diagonal, over the share: split\n", bytes * 1e-9, Pr);
            b.P = Pr;
            return PS_SPLIT;
        }
    }
    {
        const int rc = b.place(rt, Pneed, cap > 0);
        // several runtimes share the device and sized their pools at different times: when the matrices cannot be had even after the
        // idle pools were taken back (DBuf::ensure), a caller that can split does so instead of failing
        if (rc == PS_ERR_NOMEM && cap > 0) { b.P = std::min(b.Pmax, std::max(64, ((Pneed + 63) / 64) * 64)); return PS_SPLIT; }
        PS_TRY(rc);
    }
    if (rt->prof_on) { rt->prof["fill"].bytes += b.fill_alg_bytes(); rt->prof["fill"].units += (double)b.d.njobs * b.ndir; }
    PS_TRY(launch_fill(rt, b.d, b.jobs, b.ndir, b.maxS, b.P, b.ncols));
    PS_TRY(launch_backtrace(rt, b.d, b.maxn, b.moves));
    PS_TRY(launch_updaterefs(rt, b.d));
    return PS_OK;
}

// Slots per anti-diagonal realign() will probably need for this AlignData (guess_slots_w, ps_plan.h).
// Only a guess (ragged remapped alignments, few levels per base: up to 2W + 1): callers that size batches on it pass realign() a cap
// and split when it answers PS_SPLIT.  PORESEQ_DEBUG_GUESS_P overrides it (tests: a wrong guess).
int guess_slots(const Align* a) {
    static const int dbg = getenv("PORESEQ_DEBUG_GUESS_P") ? atoi(getenv("PORESEQ_DEBUG_GUESS_P")) : 0;
    return dbg > 0 ? std::min(1024, std::max(64, dbg)) : guess_slots_w(a->par.realign_width);
}

// What the events of one AlignData will probably take on the device when each takes `ndir` sweeps, and what a lock-step call may
// take of it (in_share_chunks, ps_host.h)
double share_need(const Align* a, int ndir) {
    const int P = guess_slots(a);
    double add = 0;
    for (int e = 0; e < a->E; e++)
        add += ndir == 1 ? fwd_job_bytes(a, a->n[e], (int)a->states.size()) : matrix_bytes((int64_t)a->n[e] + (int64_t)a->states.size() + 1, P, ndir);
    return add;
}
double share_cap(int ndir) { return ndir == 2 ? dense_cap_bytes() : device_share_bytes(); }

// One greedy pass of MakeMutations (ps_greedy.h: sort, apply, defer, shift) on the AlignData's sequence
static int greedy_apply(Align* a, std::vector<Mut>& muts, std::vector<Mut>* later, bool talk) {
    bool changed = false;
    const int nb = greedy_apply(a->bases, muts, later, talk, a->par.verbose, &changed);
    if (changed) a->states = states_of(a->bases);
    return nb;
}

// MakeMutations for several AlignData in lock-step: the greedy passes run on host threads, every round of re-scoring
// is one batched ScoreMutations over the AlignData that still have more than ten disabled edits
int make_mutations_multi(Runtime* rt, const std::vector<Align*>& as, std::vector<std::vector<Mut>> muts, std::vector<int>* nbases) {
    Tick tk("make_mutations");
    const int R = (int)as.size();
    nbases->assign(R, 0);
    for (Align* a : as) a->keep_valid = a->restore_due = false;   // MakeMutations belongs to the calls that write their refs back: nothing to go back to
    std::vector<int> active(R);
    std::iota(active.begin(), active.end(), 0);
    std::vector<std::vector<Mut>> later(R);
    while (!active.empty()) {
        par_for((int)active.size(), [&](int q) {
            const int k = active[q];
            (*nbases)[k] += greedy_apply(as[k], muts[k], &later[k], R == 1 && as[k]->par.verbose);
        });
        tk.lap("greedy apply");
        std::vector<int> next;
        for (int k : active) if (later[k].size() > 10) next.push_back(k);
        if (next.empty()) break;
        std::vector<EditReq> rq(next.size());
        for (size_t q = 0; q < next.size(); q++) { rq[q].a = as[next[q]]; rq[q].muts = &later[next[q]]; rq[q].out = &muts[next[q]]; }
        PS_TRY(score_edits(rt, EditKind::List, rq.data(), rq.size()));
        active.swap(next);
    }
    return PS_OK;
}

int make_mutations(Runtime* rt, Align* a, std::vector<Mut> muts, int* nbases) {
    std::vector<int> nb;
    std::vector<std::vector<Mut>> in(1);
    in[0] = std::move(muts);
    PS_TRY(make_mutations_multi(rt, {a}, std::move(in), &nb));
    *nbases = nb[0];
    return PS_OK;
}

}  // namespace ps
