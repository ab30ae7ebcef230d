// ps_host.cpp — host side of libporeseq_hip.so above the runtime: sequences, AlignData, alignment batches and realign() (which
// fill runs for a batch, in which form), and the refinement-loop logic that the reference keeps in C++ above its Alignment class
// (cpp/MakeMutations.cpp, cpp/EventUtil.cpp): ScoreAlignments and MakeMutations.  ScoreMutations and its reductions — the edit-scoring
// chain — are in ps_score.cpp, the edit plans in ps_editplan.h, FindMutations in ps_find.cpp.  The runtime, its streams and par_for
// are in ps_runtime.cpp; device memory — pools, shares, slabs, the AlignData slab cache — in ps_mem.cpp, its arithmetic in ps_plan.h.
// All dynamic-programming arithmetic runs in the HIP kernels (ps_kernels.hip, ps_edit.hip, ps_sw.hip,
// ps_viterbi.hip); there is no CPU implementation of it in this library.
#include "ps_host.h"
#include "ps_sane.h"

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

// ------------------------------------------------------------------------------------------ AlignData
Align::~Align() {
    if (d_keep) (void)hipFree(d_keep);
    align_slab_give(slab, slab_cap, last_stream);   // (back to the cache of ps_mem.cpp, or freed)
}

int Align::create(Runtime* rt, const char* seq, int64_t seq_len, int32_t n_events, const int64_t* level_off,
                  const double* mean, const double* stdv, const double* ref_align, const double* ref_like,
                  const double* model, const double* trans, const char* evseq, const int64_t* evseq_off,
                  const ps_params* params) {
    bases.assign(seq, (size_t)seq_len);
    states = states_of(bases);
    if (params) par = *params;
    E = n_events;
    n.resize(E); off.resize(E + 1);
    for (int e = 0; e <= E; e++) off[e] = E ? level_off[e] - level_off[0] : 0;
    for (int e = 0; e < E; e++) { n[e] = (int)(off[e + 1] - off[e]); if (n[e] < 0) return fail(PS_ERR_BAD_ARG, "level_off not monotone"); }
    ntot = E ? off[E] : 0;
    const int64_t base = E ? level_off[0] : 0;
    evseqs.resize(E);
    if (evseq && evseq_off) for (int e = 0; e < E; e++) evseqs[e].assign(evseq + evseq_off[e], evseq + evseq_off[e + 1]);
    // +infinity emissions are refused, the other values outside the reference's domain marked (ps_sane.h)
    nonfinite.clear();
    {
        char msg[200];
        if (offset_refused(par.lik_offset)) { snprintf(msg, sizeof msg, "lik_offset %g is not finite", par.lik_offset); return fail(PS_ERR_BAD_ARG, msg); }
        for (int e = 0; e < E; e++) {
            for (int64_t t = off[e]; t < off[e + 1]; t++) {
                const double m = mean[base + t], sd = stdv[base + t];
                if (level_plus_inf(sd)) {
                    snprintf(msg, sizeof msg, "event %d, level %lld: stdv %g (the emission of the mirrored row is +infinity)", e, (long long)(t - off[e]), sd);
                    return fail(PS_ERR_BAD_ARG, msg);
                }
                if (nonfinite.empty() && level_nonfinite(m, sd)) {
                    snprintf(msg, sizeof msg, "event %d, level %lld: mean %g, stdv %g", e, (long long)(t - off[e]), m, sd);
                    nonfinite = msg;
                }
            }
        }
    }
    h_mean.assign(mean + base, mean + base + ntot);
    h_stdv.assign(stdv + base, stdv + base + ntot);
    h_ra.assign(ref_align + base, ref_align + base + ntot);
    h_rl.assign(ref_like + base, ref_like + base + ntot);
    host_refs_valid = true;
    // derived model columns with the host libm, exactly as ModelData::setData / setParams (cpp/EventData.h:48-73)
    std::vector<double> lsd(ntot), mdl((size_t)E * 6 * NS), tr((size_t)E * 4);
    for (int64_t t = 0; t < ntot; t++) lsd[t] = std::log(h_stdv[t]);
    for (int e = 0; e < E; e++) {
        const double* src = model + (size_t)e * 4 * NS;
        double* dst = mdl.data() + (size_t)e * 6 * NS;
        for (int k = 0; k < NS; k++) {
            const double lm = src[k], ls = src[NS + k], sm = src[2 * NS + k], ss = src[3 * NS + k];
            const double lam = model_lambda(sm, ss);
            if (model_row_plus_inf(ls, lam) || (nonfinite.empty() && model_row_nonfinite(lm, ls, sm, lam))) {   // (rare: the message is built only then)
                char msg[200];
                snprintf(msg, sizeof msg, "event %d, model row %d: level_mean %g, level_stdv %g, sd_mean %g, sd_stdv %g", e, k, lm, ls, sm, ss);
                if (model_row_plus_inf(ls, lam)) return fail(PS_ERR_BAD_ARG, std::string(msg) + " (its emissions are +infinity)");
                nonfinite = msg;
            }
            dst[k] = lm; dst[NS + k] = ls; dst[2 * NS + k] = std::log(ls);
            dst[3 * NS + k] = sm; dst[4 * NS + k] = lam; dst[5 * NS + k] = std::log(lam);
        }
        for (int k = 0; k < 4; k++) tr[e * 4 + k] = std::log(trans[e * 4 + k]);
    }
    h_model = mdl;
    h_trans = tr;
    // k_fill's tables: model rows with the reciprocals of the two model divisors, level records per direction with the
    // reciprocal of the level stdv (correctly rounded: host IEEE division)
    std::vector<double> mdl8((size_t)E * (MODEL_ROW_BYTES / 8) * NS), lev((size_t)2 * 4 * std::max<int64_t>(ntot, 1));
    fastdiv = true;
    for (int e = 0; e < E; e++) {
        const double* d6 = mdl.data() + (size_t)e * 6 * NS;
        double* d8 = mdl8.data() + (size_t)e * (MODEL_ROW_BYTES / 8) * NS;
        for (int k = 0; k < NS; k++) {
            const double lm = d6[k], ls = d6[NS + k], sm = d6[3 * NS + k], lam = d6[4 * NS + k];
            double* r8 = d8 + (size_t)k * (MODEL_ROW_BYTES / 8);
            r8[0] = lm; r8[1] = 1.0 / ls; r8[2] = ls; r8[3] = d6[2 * NS + k];
            r8[4] = sm; r8[5] = 1.0 / sm; r8[6] = lam; r8[7] = d6[5 * NS + k];
            if (!sane_model_row(lm, ls, sm, lam)) fastdiv = false;   // (ps_sane.h: the range, and why)
        }
        const int64_t o = off[e];
        const int ne = n[e];
        for (int i = 1; i <= ne; i++) {
            double* f = lev.data() + 4 * (o + i - 1);
            double* bk = lev.data() + 4 * (ntot + o + i - 1);
            const double l3 = 3 * lsd[o + ne - i];
            f[0] = h_mean[o + i - 1]; f[1] = h_stdv[o + i - 1]; f[2] = l3; f[3] = 1.0 / h_stdv[o + i - 1];
            bk[0] = h_mean[o + ne - i]; bk[1] = h_stdv[o + ne - i]; bk[2] = l3; bk[3] = 1.0 / h_stdv[o + ne - i];
        }
    }
    for (int64_t t = 0; t < ntot; t++)
        if (!sane_level(h_mean[t], h_stdv[t])) fastdiv = false;
    if (getenv("PORESEQ_EXACT_DIV")) fastdiv = false;   // tests: the IEEE-division build of every kernel that computes emissions
    // one slab: mean, stdv, lsd, ra, rl, ri [ntot each] | model | trans | out
    const size_t nlev = (size_t)std::max<int64_t>(ntot, 1);
    const size_t bytes = (6 + 8) * nlev * sizeof(double) + (mdl.size() + mdl8.size() + tr.size() + 2) * sizeof(double) + 256 +
                         (size_t)std::max(E, 1) * sizeof(JobOut) + 64 * 16;
    PS_TRY(align_slab_take(rt, bytes, &slab, &slab_cap));
    last_stream = (void*)rt->stream;
    // the slab is filled by ONE host-to-device copy: its image is assembled in pinned staging memory first (ten copies and a memset per
    // region before: 3 000 of a bench step's copy commands)
    char* img = (char*)rt->stage.alloc(bytes);
    if (!img) return fail(PS_ERR_NOMEM, "hipHostMalloc (staging arena)");
    memset(img, 0, bytes);
    char* p = (char*)slab;
    auto carve = [&](size_t b) { char* r = p; p += (b + 63) / 64 * 64; return r; };
    auto put = [&](const void* dev, const void* src, size_t b) { if (b) memcpy(img + ((const char*)dev - (const char*)slab), src, b); };
    d_mean = (double*)carve(nlev * 8); d_stdv = (double*)carve(nlev * 8); d_lsd = (double*)carve(nlev * 8);
    d_ra = (double*)carve(nlev * 8); d_rl = (double*)carve(nlev * 8); d_ri = (double*)carve(nlev * 8);
    d_model = (double*)carve(std::max<size_t>(mdl.size(), 1) * 8); d_trans = (double*)carve(std::max<size_t>(tr.size(), 1) * 8);
    d_out = (JobOut*)carve((size_t)std::max(E, 1) * sizeof(JobOut));
    d_model8 = (double*)carve(std::max<size_t>(mdl8.size(), 1) * 8);
    d_lev[0] = (double*)carve(4 * nlev * 8); d_lev[1] = (double*)carve(4 * nlev * 8);
    if (ntot) {
        put(d_mean, h_mean.data(), ntot * 8); put(d_stdv, h_stdv.data(), ntot * 8); put(d_lsd, lsd.data(), ntot * 8);
        put(d_ra, h_ra.data(), ntot * 8); put(d_rl, h_rl.data(), ntot * 8);
        put(d_lev[0], lev.data(), 4 * ntot * 8); put(d_lev[1], lev.data() + 4 * ntot, 4 * ntot * 8);
    }
    if (E) { put(d_model, mdl.data(), mdl.size() * 8); put(d_trans, tr.data(), tr.size() * 8); put(d_model8, mdl8.data(), mdl8.size() * 8); }
    PS_HIP(hipMemcpyAsync(slab, img, (size_t)(p - (char*)slab), hipMemcpyHostToDevice, rt->stream));   // (d_out: zeros)
    PS_HIP(hipStreamSynchronize(rt->stream));
    // EventData::setData ends with updaterefs() (cpp/EventData.h:223)
    Batch b;
    PS_TRY(base_batch(rt, &b, 1, 0));
    PS_TRY(launch_updaterefs(rt, b.d));
    PS_HIP(hipStreamSynchronize(rt->stream));
    return PS_OK;
}

int Align::base_batch(Runtime* rt, Batch* b, int ndir, int lb_extra) {
    std::vector<JobSpec> specs(E);
    for (int e = 0; e < E; e++) specs[e] = job(e);
    return b->build(rt, specs, ndir, lb_extra);
}

// event e against this AlignData's own sequence, with the event's own reference arrays and result record
JobSpec Align::job(int e) {
    JobSpec s;
    s.a = this; s.ev = e; s.states = &states;
    s.ra = d_ra + off[e]; s.rl = d_rl + off[e]; s.ri = d_ri + off[e];
    s.out = d_out + e;
    return s;
}
JobSpec Align::job(int e, const std::vector<int>* other, double* ra, double* rl, double* ri, JobOut* out) {
    JobSpec s = job(e);   // the event's data; the other sequence's states and the alignment to it on top
    s.states = other;
    s.ra = ra + off[e]; s.rl = rl + off[e]; s.ri = ri + off[e];
    s.out = out;
    return s;
}

// device -> host mirror of ref_align / ref_like in two halves, so that several AlignData can share one synchronisation
int Align::refs_to_host_async(Runtime* rt) {
    pend_ra = nullptr; pend_rl = nullptr;
    if (host_refs_valid || !ntot) { host_refs_valid = true; return PS_OK; }
    last_stream = (void*)rt->stream;
    PS_TRY(rt->down(&pend_ra, d_ra, (size_t)ntot));
    PS_TRY(rt->down(&pend_rl, d_rl, (size_t)ntot));
    return PS_OK;
}
void Align::refs_finish() {   // after the stream has been synchronised
    if (pend_ra) { memcpy(h_ra.data(), pend_ra, ntot * 8); memcpy(h_rl.data(), pend_rl, ntot * 8); }
    pend_ra = nullptr; pend_rl = nullptr;
    host_refs_valid = true;
}
int Align::refs_to_host(Runtime* rt) {
    PS_TRY(refs_to_host_async(rt));
    if (pend_ra) PS_HIP(hipStreamSynchronize(rt->stream));
    refs_finish();
    return PS_OK;
}

// ps_align_keep_refs / ps_align_new_call (include/poreseq_hip.h): d_ra and d_rl lie next to each other in the slab
// (Align::create carves them in this order), one copy each way
int Align::keep_refs(Runtime* rt) {
    if (!ntot) return PS_OK;
    if (keep_valid) { restore_due = true; return PS_OK; }   // (kept before and restored by the last new_call: the refs are the kept ones)
    const size_t span = (size_t)(d_rl - d_ra) + (size_t)ntot;
    if (!d_keep) PS_HIP(hipMalloc((void**)&d_keep, span * sizeof(double)));
    last_stream = (void*)rt->stream;
    PS_HIP(hipMemcpyAsync(d_keep, d_ra, span * sizeof(double), hipMemcpyDeviceToDevice, rt->stream));
    PS_HIP(hipStreamSynchronize(rt->stream));
    keep_valid = true;
    restore_due = true;
    return PS_OK;
}
int Align::restore_refs(Runtime* rt) {
    if (!keep_valid || !restore_due || !ntot) return PS_OK;
    restore_due = false;
    const size_t span = (size_t)(d_rl - d_ra) + (size_t)ntot;
    last_stream = (void*)rt->stream;
    PS_HIP(hipMemcpyAsync(d_ra, d_keep, span * sizeof(double), hipMemcpyDeviceToDevice, rt->stream));
    host_refs_valid = false;
    Batch b;   // ref_index, refstart and refend follow ref_align (k_updaterefs), as after EventData::setData
    PS_TRY(base_batch(rt, &b, 1, 0));
    PS_TRY(launch_updaterefs(rt, b.d));
    PS_HIP(hipStreamSynchronize(rt->stream));
    return PS_OK;
}

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
    PS_TRY(launch_backtrace(rt, b.d, b.maxn));
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

// The scores of a batch's jobs, gathered into one array on the device and enqueued for one copy back (instead of one per AlignData)
int gather_best(Runtime* rt, const Batch& b, double** best) {
    DBuf& gb = rt->buf("best");
    PS_TRY(gb.ensure(b.jobs.size() * sizeof(double)));
    PS_TRY(launch_gather_best(rt, b.d, gb.as<double>()));
    return rt->down(best, gb.p, b.jobs.size());
}

// ScoreAlignments, cpp/MakeMutations.cpp:148-195, for several AlignData in one launch chain (independent regions in lock-step)
int score_alignments_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<double*>& scores, const std::vector<double*>& likes) {
    auto sub = [&](size_t k0, size_t k1) {   // regions k0 .. k1 - 1 as a call of their own
        return score_alignments_multi(rt, std::vector<Align*>(as.begin() + k0, as.begin() + k1), std::vector<double*>(scores.begin() + k0, scores.begin() + k1),
                                      std::vector<double*>(likes.begin() + k0, likes.begin() + k1));
    };
    auto need = [&](size_t k) { return share_need(as[k], 1); };
    if (over_share(as.size(), 1, need)) return in_share_chunks(as.size(), 1, need, sub);   // more matrices than this runtime's share of the device
    std::vector<JobSpec> specs;
    for (Align* a : as)
        for (int e = 0; e < a->E; e++) specs.push_back(a->job(e));
    if (specs.empty()) return PS_OK;
    Batch b;
    PS_TRY(b.build(rt, specs, 1, 0));
    {
        const int rc = realign(rt, b, as.size() > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0);
        if (rc == PS_SPLIT) return in_halves(as.size(), sub);   // bands wider than share_need guessed: two halves, one after the other
        PS_TRY(rc);
    }
    for (Align* a : as) a->host_refs_valid = false;
    double* best = nullptr;
    PS_TRY(gather_best(rt, b, &best));
    bool any_likes = false;
    for (size_t k = 0; k < as.size(); k++) if (likes[k]) { any_likes = true; PS_TRY(as[k]->refs_to_host_async(rt)); }
    PS_HIP(hipStreamSynchronize(rt->stream));
    {
        size_t j = 0;
        for (size_t k = 0; k < as.size(); k++)
            for (int e = 0; e < as[k]->E; e++) scores[k][e] = std::max(best[j++], 0.0);  // Alignment::getMax, cpp/Alignment.h:127-130
    }
    if (any_likes)
        par_for((int)as.size(), [&](int k) {
            Align* a = as[k];
            if (!likes[k]) return;
            a->refs_finish();
            for (int e = 0; e < a->E; e++) accumulate_likes(a->h_ra.data() + a->off[e], a->h_rl.data() + a->off[e], a->n[e], (int)a->states.size(), likes[k]);
        });
    return PS_OK;
}

int score_alignments(Runtime* rt, Align* a, double* scores, double* likes) {
    if (!a->E) return PS_OK;
    return score_alignments_multi(rt, {a}, {scores}, {likes});
}

// The descriptors of k_align_stats and k_kmer_stats for the AlignData `as`, whose events are the jobs of `b` in order: one StatJob
// per event, one StatRegion per AlignData.  groups (k_kmer_stats; null otherwise): per AlignData the events' group ids and the
// number of groups; the regions' table rows follow each other.  Returns the levels of all events.
static double stat_descriptors(const std::vector<Align*>& as, const Batch& b, const std::vector<const int32_t*>* groups, const std::vector<int>* ngroups,
                               std::vector<StatJob>* sj, std::vector<StatRegion>* sr, int* maxE) {
    sj->assign(b.jobs.size(), StatJob());
    sr->assign(as.size(), StatRegion());
    *maxE = 0;
    double levels = 0;
    size_t q = 0;
    int tab = 0;
    for (size_t k = 0; k < as.size(); k++) {
        const Align* a = as[k];
        StatRegion& r = (*sr)[k];
        r.job0 = (int)q; r.njobs = a->E; r.ngroups = groups ? (*ngroups)[k] : 0; r.tab0 = tab;
        tab += r.ngroups;
        *maxE = std::max(*maxE, a->E);
        for (int e = 0; e < a->E; e++, q++) {
            const JobD& j = b.jobs[q];
            StatJob& s = (*sj)[q];
            s.ra = j.ra; s.mean = a->d_mean + a->off[e]; s.stdv = a->d_stdv + a->off[e]; s.model = a->d_model + (size_t)e * 6 * NS;
            s.st = j.st; s.n = j.n0; s.S = j.C;
            s.grp = groups ? (*groups)[k][e] : 0; s.pad = 0;
            levels += j.n0;
        }
    }
    return levels;
}

// ps_align_stats / ps_batch_align_stats (include/poreseq_hip.h): with `re`, ScoreAlignments' chain as above and then k_align_stats
// over the refs the backtrace just wrote; without it k_align_stats over the refs the handles hold, and no DP.  Either way one
// launch of it for all AlignData, and scores and records return in one copy.  scores[k] may be null.
int align_stats_multi(Runtime* rt, const std::vector<Align*>& as, bool re, const std::vector<double*>& scores, const std::vector<ps_event_stats*>& stats) {
    auto sub = [&](size_t k0, size_t k1) {   // regions k0 .. k1 - 1 as a call of their own
        return align_stats_multi(rt, std::vector<Align*>(as.begin() + k0, as.begin() + k1), re, std::vector<double*>(scores.begin() + k0, scores.begin() + k1),
                                 std::vector<ps_event_stats*>(stats.begin() + k0, stats.begin() + k1));
    };
    auto need = [&](size_t k) { return share_need(as[k], 1); };
    if (re && over_share(as.size(), 1, need)) return in_share_chunks(as.size(), 1, need, sub);   // (cut between AlignData, as ScoreAlignments is)
    std::vector<JobSpec> specs;
    for (Align* a : as)
        for (int e = 0; e < a->E; e++) specs.push_back(a->job(e));
    if (specs.empty()) return PS_OK;
    Batch b;   // (also without a realignment: it puts every sequence's states on the device)
    PS_TRY(b.build(rt, specs, 1, 0));
    if (re) {
        const int rc = realign(rt, b, as.size() > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0);
        if (rc == PS_SPLIT) return in_halves(as.size(), sub);
        PS_TRY(rc);
        for (Align* a : as) a->host_refs_valid = false;
    }
    const size_t nj = specs.size();
    std::vector<StatJob> sj;
    std::vector<StatRegion> sr;
    int maxE = 0;
    const double bytes = 16.0 * stat_descriptors(as, b, nullptr, nullptr, &sj, &sr, &maxE) + (double)nj * sizeof(ps_event_stats);
    // descriptors in; records and, behind them, the scores out
    const size_t in_jobs = nj * sizeof(StatJob), in_bytes = in_jobs + sr.size() * sizeof(StatRegion);
    const size_t out_recs = nj * sizeof(ps_event_stats), out_bytes = out_recs + (re ? nj * sizeof(double) : 0);
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(in_bytes));
    PS_TRY(dout.ensure(out_bytes));
    PS_TRY(rt->up(din.p, sj.data(), in_jobs));
    PS_TRY(rt->up((char*)din.p + in_jobs, sr.data(), sr.size() * sizeof(StatRegion)));
    PS_TRY(launch_align_stats(rt, din.as<StatJob>(), (const StatRegion*)((char*)din.p + in_jobs), (int)sr.size(), maxE, bytes, dout.as<ps_event_stats>()));
    if (re) PS_TRY(launch_gather_best(rt, b.d, (double*)((char*)dout.p + out_recs)));
    void* back = nullptr;
    PS_TRY(rt->down(&back, dout.p, out_bytes));
    PS_HIP(hipStreamSynchronize(rt->stream));
    const ps_event_stats* recs = (const ps_event_stats*)back;
    const double* best = (const double*)((const char*)back + out_recs);
    size_t q = 0;
    for (size_t k = 0; k < as.size(); k++)
        for (int e = 0; e < as[k]->E; e++, q++) {
            stats[k][e] = recs[q];
            if (re && scores[k]) scores[k][e] = std::max(best[q], 0.0);   // Alignment::getMax, cpp/Alignment.h:127-130
        }
    return PS_OK;
}

// ps_kmer_stats / ps_batch_kmer_stats (include/poreseq_hip.h): align_stats_multi's shape — the same Batch, the same optional
// realignment with the same split rules, one launch of k_kmer_stats for all AlignData, tables and scores back in one copy.  A batch
// whose tables (48 KiB per group) exceed this runtime's share is cut between AlignData as well.  Every as[k] has events or not;
// tables[k] has ngroups[k] x NS cells and is written in full.
int kmer_stats_multi(Runtime* rt, const std::vector<Align*>& as, bool re, const std::vector<const int32_t*>& groups, const std::vector<int>& ngroups,
                     const std::vector<double*>& scores, const std::vector<ps_kmer_cell*>& tables) {
    auto sub = [&](size_t k0, size_t k1) {   // regions k0 .. k1 - 1 as a call of their own
        return kmer_stats_multi(rt, std::vector<Align*>(as.begin() + k0, as.begin() + k1), re, std::vector<const int32_t*>(groups.begin() + k0, groups.begin() + k1),
                                std::vector<int>(ngroups.begin() + k0, ngroups.begin() + k1), std::vector<double*>(scores.begin() + k0, scores.begin() + k1),
                                std::vector<ps_kmer_cell*>(tables.begin() + k0, tables.begin() + k1));
    };
    size_t rows = 0;
    int maxG = 0;
    for (int g : ngroups) { rows += (size_t)g; maxG = std::max(maxG, g); }
    const size_t out_tabs = rows * NS * sizeof(ps_kmer_cell);
    if (as.size() > 1 && (double)out_tabs > device_share_bytes()) return in_halves(as.size(), sub);
    auto need = [&](size_t k) { return share_need(as[k], 1); };
    if (re && over_share(as.size(), 1, need)) return in_share_chunks(as.size(), 1, need, sub);   // (cut between AlignData, as ScoreAlignments is)
    std::vector<JobSpec> specs;
    for (Align* a : as)
        for (int e = 0; e < a->E; e++) specs.push_back(a->job(e));
    if (specs.empty()) {
        for (size_t k = 0; k < as.size(); k++) memset(tables[k], 0, (size_t)ngroups[k] * NS * sizeof(ps_kmer_cell));
        return PS_OK;
    }
    Batch b;   // (also without a realignment: it puts every sequence's states on the device)
    PS_TRY(b.build(rt, specs, 1, 0));
    if (re) {
        const int rc = realign(rt, b, as.size() > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0);
        if (rc == PS_SPLIT) return in_halves(as.size(), sub);
        PS_TRY(rc);
        for (Align* a : as) a->host_refs_valid = false;
    }
    const size_t nj = specs.size();
    std::vector<StatJob> sj;
    std::vector<StatRegion> sr;
    int maxE = 0;
    const double bytes = 24.0 * stat_descriptors(as, b, &groups, &ngroups, &sj, &sr, &maxE) + (double)out_tabs;
    // descriptors in; tables and, behind them, the scores out
    const size_t in_jobs = nj * sizeof(StatJob), in_bytes = in_jobs + sr.size() * sizeof(StatRegion);
    const size_t out_bytes = out_tabs + (re ? nj * sizeof(double) : 0);
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(in_bytes));
    PS_TRY(dout.ensure(out_bytes));
    PS_TRY(rt->up(din.p, sj.data(), in_jobs));
    PS_TRY(rt->up((char*)din.p + in_jobs, sr.data(), sr.size() * sizeof(StatRegion)));
    PS_TRY(launch_kmer_stats(rt, din.as<StatJob>(), (const StatRegion*)((char*)din.p + in_jobs), (int)sr.size(), maxG, bytes, dout.as<ps_kmer_cell>()));
    if (re) PS_TRY(launch_gather_best(rt, b.d, (double*)((char*)dout.p + out_tabs)));
    void* back = nullptr;
    PS_TRY(rt->down(&back, dout.p, out_bytes));
    PS_HIP(hipStreamSynchronize(rt->stream));
    const ps_kmer_cell* tabs = (const ps_kmer_cell*)back;
    const double* best = (const double*)((const char*)back + out_tabs);
    size_t q = 0;
    for (size_t k = 0; k < as.size(); k++) {
        memcpy(tables[k], tabs + (size_t)sr[k].tab0 * NS, (size_t)ngroups[k] * NS * sizeof(ps_kmer_cell));
        for (int e = 0; e < as[k]->E; e++, q++)
            if (re && scores[k]) scores[k][e] = std::max(best[q], 0.0);   // Alignment::getMax, cpp/Alignment.h:127-130
    }
    return PS_OK;
}

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
