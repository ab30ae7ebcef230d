// ps_host.cpp — host side of libporeseq_hip.so above the runtime: sequences, AlignData, alignment batches and realign() (which
// fill runs for a batch, in which form), and the refinement-loop logic that the reference keeps in C++ above its Alignment class
// (cpp/MakeMutations.cpp, cpp/FindMutations.cpp, cpp/EventUtil.cpp, cpp/Sequence.h): ScoreAlignments, ScoreMutations with its edit
// plans, FindPointMutations, MakeMutations.  The runtime, its streams and par_for are in ps_runtime.cpp; device memory — pools,
// shares, slabs, the AlignData slab cache — in ps_mem.cpp, its arithmetic in ps_plan.h.
// All dynamic-programming arithmetic runs in the HIP kernels (ps_kernels.hip, ps_sw.hip,
// ps_viterbi.hip); there is no CPU implementation of it in this library.
#include "ps_host.h"
#include "ps_sane.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <numeric>
#include <thread>

namespace ps {

// ------------------------------------------------------------------------------------------ sequences
// Sequence::populateStates, cpp/Sequence.h:64-100
std::vector<int> states_of(const std::string& bases) {
    std::vector<int> st;
    if (bases.size() < 5) return st;
    auto code = [](char c) -> int { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : (int)(signed char)c; };
    int cur = 0;
    for (int i = 0; i < 4; i++) cur = (cur << 2) + code(bases[i]);
    st.resize(bases.size() - 4);
    for (size_t i = 4; i < bases.size(); i++) {
        if (code(bases[i - 4]) < 4) { cur = (NS - 1) & ((cur << 2) + code(bases[i])); st[i - 4] = cur; }
        else { cur = 0; st[i - 4] = -1; }
    }
    return st;
}

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
static int sparse_min() { return g_sparse_min.load() >= 0 ? g_sparse_min.load() : sparse_min_default(); }
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

// Where the sub-batch of AlignData that starts at as[k0] ends when each event takes `ndir` sweeps: everything if it fits this
// runtime's device share; otherwise the fewest sub-batches that fit, of about equal size (share_cut, ps_plan.h)
static size_t fit_share(const std::vector<Align*>& as, size_t k0, int ndir) {
    const double cap = ndir == 2 ? dense_cap_bytes() : device_share_bytes();   // (full forward + backward matrices live in a slab)
    auto need = [&](size_t k) {
        const Align* a = as[k];
        const int P = guess_slots(a);
        double add = 0;
        for (int e = 0; e < a->E; e++)
            add += ndir == 1 ? fwd_job_bytes(a, a->n[e], (int)a->states.size()) : matrix_bytes((int64_t)a->n[e] + (int64_t)a->states.size() + 1, P, ndir);
        return add;
    };
    return share_cut(k0, as.size(), cap, need);
}

// regions k0 .. k1 - 1 of a lock-step call as calls of their own, sub(k0, k1), one after the other: the sub-batches that fit this
// runtime's share (fit_share), or two halves (a call whose bands came out wider than guessed)
template <class Sub> static int in_share_chunks(const std::vector<Align*>& as, int ndir, Sub&& sub) {
    for (size_t k0 = 0; k0 < as.size();) {
        const size_t k1 = fit_share(as, k0, ndir);
        PS_TRY(sub(k0, k1));
        k0 = k1;
    }
    return PS_OK;
}
template <class Sub> static int in_halves(size_t n, Sub&& sub) {
    const size_t h = n / 2;
    PS_TRY(sub(0, h));
    return sub(h, n);
}

// ScoreAlignments, cpp/MakeMutations.cpp:148-195, for several AlignData in one launch chain (independent regions in lock-step)
int score_alignments_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<double*>& scores, const std::vector<double*>& likes) {
    auto sub = [&](size_t k0, size_t k1) {   // regions k0 .. k1 - 1 as a call of their own
        return score_alignments_multi(rt, std::vector<Align*>(as.begin() + k0, as.begin() + k1), std::vector<double*>(scores.begin() + k0, scores.begin() + k1),
                                      std::vector<double*>(likes.begin() + k0, likes.begin() + k1));
    };
    if (fit_share(as, 0, 1) < as.size()) return in_share_chunks(as, 1, sub);   // more matrices than this runtime's share of the device
    std::vector<JobSpec> specs;
    for (Align* a : as)
        for (int e = 0; e < a->E; e++) specs.push_back(a->job(e));
    if (specs.empty()) return PS_OK;
    Batch b;
    PS_TRY(b.build(rt, specs, 1, 0));
    {
        const int rc = realign(rt, b, as.size() > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0);
        if (rc == PS_SPLIT) return in_halves(as.size(), sub);   // bands wider than fit_share guessed: two halves, one after the other
        PS_TRY(rc);
    }
    // the jobs' scores, gathered into one array on the device: one copy back instead of one per AlignData
    for (Align* a : as) a->host_refs_valid = false;
    double* best = nullptr;
    {
        DBuf& gb = rt->buf("best");
        PS_TRY(gb.ensure(specs.size() * sizeof(double)));
        PS_TRY(launch_gather_best(rt, b.d, gb.as<double>()));
        PS_TRY(rt->down(&best, gb.p, specs.size()));
    }
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

// the `likes` loop of ScoreAlignments, cpp/MakeMutations.cpp:168-189 (one event)
void accumulate_likes(const double* ra, const double* rl, int n, int C, double* likes) {
    double last = 0;
    int refind = 1;
    for (int t = 0; t < n; t++) {
        if (ra[t] > 0) {
            for (int k = refind; k < ra[t]; k++) likes[k + 1] += last;
            last = rl[t];
            refind = (int)ra[t];
        }
    }
    for (int64_t k = refind; k < (int64_t)C + 3; k++) likes[k + 1] += last;
}

// states of the edited sequence at columns sidx+1 .. sidx+ncol, without building the whole sequence;
// equals Sequence(original, mut).states there (cpp/Sequence.h:37-100).  A 12-base look-back flushes
// every effect of earlier non-ACGT characters (they reach at most 8 states ahead).
static void edited_window(const std::string& b, const Mut& m, int sidx, int ncol, int* out) {
    const bool copy = (size_t)m.start >= b.size();
    const int64_t L = (int64_t)b.size();
    const int64_t cut = copy ? L : std::min<int64_t>(L, (int64_t)m.start + (int64_t)m.orig.size());
    const int64_t mlen = copy ? 0 : (int64_t)m.mut.size();
    const int64_t Lm = copy ? L : (int64_t)m.start + mlen + (L - cut);
    auto at = [&](int64_t p) -> char {
        if (copy || p < m.start) return b[p];
        if (p < m.start + mlen) return m.mut[p - m.start];
        return b[cut + (p - m.start - mlen)];
    };
    const int64_t lo = std::max<int64_t>(0, (int64_t)sidx - 12);
    const int64_t hi = std::min<int64_t>(Lm, (int64_t)sidx + ncol + 4);
    std::string w;
    w.reserve(hi - lo);
    for (int64_t p = lo; p < hi; p++) w.push_back(at(p));
    std::vector<int> st = states_of(w);
    for (int c = 0; c < ncol; c++) {
        const int64_t k = (int64_t)sidx + c - lo;
        out[c] = (k >= 0 && k < (int64_t)st.size()) ? st[k] : -1;
    }
}

// Where FindPointMutations' list (cpp/FindMutations.cpp:200-228) keeps each position's edits: first[p] is the index of position p's
// deletion, followed by its substitutions in ACGT order without the one by the base itself, then the four insertions — 8 edits for an
// A / C / G / T base, 9 for any other character; first[n] = the length of the list.  triv[p]: table slot 1 .. 4 of the substitution
// that is not in the list, 0 when all four are.
static void point_layout(const Align* a, std::vector<int>* first, std::vector<int>* triv) {
    const size_t n = a->states.size();
    first->resize(n + 1); triv->resize(n);
    int m = 0;
    for (size_t i = 0; i < n; i++) {
        const char c = a->bases[i];
        const int t = c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : 0;
        (*first)[i] = m; (*triv)[i] = t;
        m += t ? 8 : 9;
    }
    (*first)[n] = m;
}

// the rows of an AlignData without events: every edit keeps the seed of its sum, -1e-6 (cpp/AlignUtil.h:86)
static void point_rows_seed(const std::vector<int>& triv, double* table, ps_point_best* best) {
    for (size_t p = 0; p < triv.size(); p++) {
        if (table)
            for (int q = 0; q < PT_SLOTS; q++) table[p * PT_SLOTS + q] = (triv[p] && q == triv[p]) ? std::nan("") : -1e-6;
        if (best) { best[p].margin = -1e-6; best[p].slot = 0; best[p].n_positive = 0; }
    }
}

namespace {
// host-side description of one AlignData's edit list for k_old / k_score
struct EditPlan {
    int M = 0, ncolmax = 1, extra = 0, nr0 = 0;
    std::vector<int> start, mlen, cm, ncol, skip, oldidx, states, r0s, cls[SCORE_CLASSES];
    std::vector<int> keep[2];   // per direction: kept-column index of column 0 .. C + 1, or -1 (plan_keep)
    int nkeep[2] = {0, 0};
    int rc = PS_OK;
};
}  // namespace

static void plan_edits(const Align* a, const std::vector<Mut>& muts, EditPlan* p) {
    const int M = (int)muts.size();
    p->M = M;
    for (const Mut& m : muts) if (m.start < 0) { p->rc = PS_ERR_BAD_ARG; return; }
    const int64_t L = (int64_t)a->bases.size();
    const int C = (int)a->states.size();
    const int WS = a->par.scoring_width;
    p->start.resize(M); p->mlen.resize(M); p->cm.resize(M); p->ncol.resize(M); p->skip.resize(M); p->oldidx.resize(M);
    int ncolmax = 1, extra = 0;
    for (int i = 0; i < M; i++) {
        const Mut& m = muts[i];
        p->start[i] = m.start; p->mlen[i] = (int)m.mut.size();
        p->skip[i] = (int64_t)m.start > L ? 1 : 0;  // "sanity check", cpp/MakeMutations.cpp:46-47
        const bool copy = (int64_t)m.start >= L;
        const int64_t cut = std::min<int64_t>(L, (int64_t)m.start + (int64_t)m.orig.size());
        const int64_t Lm = copy ? L : (int64_t)m.start + (int64_t)m.mut.size() + (L - cut);
        const int Cm = Lm >= 5 ? (int)(Lm - 4) : 0;
        p->cm[i] = Cm;
        const int sidx = std::max(m.start - 4, 0);
        int ncol = std::min<int64_t>((int64_t)m.mut.size() + 6, std::max<int64_t>(0, (int64_t)Cm - sidx));
        if (WS == 0 || p->skip[i]) ncol = 0;  // stripe_width 0 makes fillColumn a no-op, cpp/Alignment.cpp:118-119
        p->ncol[i] = ncol;
        ncolmax = std::max(ncolmax, ncol);
        if (!p->skip[i]) extra = std::max(extra, sidx + ncol + 1 - (C + 1));
    }
    p->ncolmax = ncolmax;
    p->extra = std::max(extra, 0) + 2;
}

// The matrix columns the scoring of this list will read (k_old / k_score, cpp/Alignment.cpp:447-512, cpp/Alignment.h:181-214):
// per edit the forward column it is spliced behind, max(start - 4, 0), the column pair of its old score, max(start - 3, 1) forward
// and C - that + 1 backward, and the backward column its target is combined with — with the kernels' own clamping.  Column 0 (the
// blank column) is never read from the records.
static void plan_keep(const Align* a, EditPlan* p) {
    const int C = (int)a->states.size();
    for (int d = 0; d < 2; d++) { p->keep[d].assign((size_t)C + 2, -1); p->nkeep[d] = 0; }
    auto clampc = [&](int c) { return (unsigned)c >= (unsigned)(C + 1) ? C : c; };
    for (int i = 0; i < p->M; i++) {
        if (p->skip[i]) continue;
        const int start = p->start[i];
        const int sidx = std::max(start - 4, 0);
        const int tcol = std::min(start + p->mlen[i] + 1, sidx + p->ncol[i]);
        const int backind = clampc(p->cm[i] - tcol + 1);
        const int r0 = std::max(start - 3, 1);
        const int raf = clampc(r0), rab = clampc(C - r0 + 1);
        const int sf = clampc(sidx);
        if (sf > 0) p->keep[0][sf] = 0;
        if (raf > 0) p->keep[0][raf] = 0;
        if (backind > 0) p->keep[1][backind] = 0;
        if (rab > 0) p->keep[1][rab] = 0;
    }
    for (int d = 0; d < 2; d++)
        for (int c = 0; c <= C + 1; c++) if (p->keep[d][c] == 0) p->keep[d][c] = p->nkeep[d]++;
}

// second half of the plan (runs on host threads while the GPU realigns): edited states, distinct r0, size classes
static void plan_tables(const Align* a, const std::vector<Mut>& muts, EditPlan* p, int nth) {
    const int M = p->M, ncolmax = p->ncolmax;
    const int64_t L = (int64_t)a->bases.size();
    p->states.assign((size_t)M * ncolmax, -1);
    {
        auto work = [&](int lo, int hi) {
            for (int i = lo; i < hi; i++)
                if (p->ncol[i] > 0) edited_window(a->bases, muts[i], std::max(muts[i].start - 4, 0), p->ncol[i], p->states.data() + (size_t)i * ncolmax);
        };
        if (M < 4096) nth = 1;   // Refine-sized lists: split over a few host threads (disjoint outputs)
        std::vector<std::thread> th;
        for (int t = 1; t < nth; t++) th.emplace_back(work, (int)((int64_t)M * t / nth), (int)((int64_t)M * (t + 1) / nth));
        work(0, (int)((int64_t)M / nth));
        for (std::thread& x : th) x.join();
    }
    std::vector<int> idx((size_t)std::max<int64_t>(L, 4) + 2, -1);   // r0 <= L - 3 for every edit that is not skipped
    for (int i = 0; i < M; i++) {
        if (p->skip[i]) { p->oldidx[i] = 0; continue; }
        const int r0 = std::max(muts[i].start - 3, 1);
        int& at = idx[r0];
        if (at < 0) { at = (int)p->r0s.size(); p->r0s.push_back(r0); }
        p->oldidx[i] = at;
    }
    p->nr0 = (int)p->r0s.size();
    for (int i = 0; i < M; i++) {
        const int nc = p->ncol[i];
        p->cls[nc <= 7 ? 4 : nc <= 8 ? 0 : nc <= 16 ? 1 : nc <= 32 ? 2 : 3].push_back(i);
    }
}

// ScoreMutations, cpp/MakeMutations.cpp:23-69, for several AlignData at once: one realign launch chain over all their
// events (forward + backward of one event share a workgroup), then the edit scoring of each
// a point-table call (point_table_multi): per AlignData the host arrays that receive its rows and its per-position records (either may
// be null); the lists are FindPointMutations' and no scored copy is made (`outs` is empty)
namespace {
struct PointOut { std::vector<double*> table; std::vector<ps_point_best*> best; };
// a support call (score_mutation_support_multi): per AlignData the events' group ids, the number of groups and the host arrays that
// receive the scores (may be null) and the [M][ngroups] records; no scored copy of the lists is made either
struct SupportOut {
    std::vector<const int32_t*> group; std::vector<int> ngroups; std::vector<double*> score; std::vector<ps_edit_support*> rec;
    // a genotype call (score_mutation_genotypes_multi) on top: per AlignData the alt fractions and the host arrays that receive the
    // [M][nfrac + 1] likelihoods and the covering-event counts (may be null); `rec` entries may then be null (no records wanted)
    bool geno = false;
    std::vector<int> nfrac; std::vector<const double*> frac; std::vector<double*> lik; std::vector<int32_t*> ncover;
};
}  // namespace
static int score_mutations_planned(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<Mut>*>& muts,
                                   const std::vector<std::vector<Mut>*>& outs, const std::vector<double*>* delta_out, std::vector<EditPlan>& plan,
                                   const PointOut* pt = nullptr, const SupportOut* sp = nullptr);

int score_mutations_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<Mut>*>& muts,
                          const std::vector<std::vector<Mut>*>& outs, const std::vector<double*>* delta_out) {
    const int R = (int)as.size();
    std::vector<EditPlan> plan(R);
    par_for(R, [&](int k) {   // (a Refine list is 80 000 edits per region: copied and sized side by side)
        *outs[k] = *muts[k];
        for (Mut& m : *outs[k]) m.score = -1e-6;
        plan_edits(as[k], *muts[k], &plan[k]);
    });
    for (int k = 0; k < R; k++) {
        if (as[k]->par.scoring_width < 0) return fail(PS_ERR_BAD_ARG, "scoring_width < 0");
        if (plan[k].rc != PS_OK) return fail(plan[k].rc, "negative mutation start");
        if (plan[k].ncolmax > 64 && as[k]->par.scoring_width > 511) return fail(PS_ERR_UNSUPPORTED, "edit longer than 58 bases with scoring_width > 511");
    }
    return score_mutations_planned(rt, as, muts, outs, delta_out, plan);
}

// `plan`: every list sized (plan_edits) and `outs` initialised — once per call: the sub-batches of a call that does not fit a slab or the
// runtime's share, and the halves of one whose bands came out wider than guessed, take their regions' plans with them (moved: the
// caller returns right behind them) instead of copying and sizing 80 000 edits per region again
static int score_mutations_planned(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<Mut>*>& muts,
                                   const std::vector<std::vector<Mut>*>& outs, const std::vector<double*>* delta_out, std::vector<EditPlan>& plan,
                                   const PointOut* pt, const SupportOut* sp) {
    Tick tk(pt ? "point_table" : sp ? (sp->geno ? "score_mutation_genotypes" : "score_mutation_support") : "score_mutations");
    const int R = (int)as.size();
    // the reference's progress line under `verbose` (cpp/MakeMutations.cpp:28-32, 55-66: "Scoring (<width>)", a dot per event, a newline);
    // a lock-step call over several AlignData has no single line to write: only the single-handle call speaks
    if (R == 1 && as[0]->par.verbose) {
        fprintf(stderr, "Scoring (%d)", (int)as[0]->par.scoring_width);
        for (int e = 0; e < as[0]->E; e++) fputc('.', stderr);
        fputc('\n', stderr);
        fflush(stderr);
    }
    // Which columns of the score matrices will the edit lists read?  A short list (FindMutations' found edits, the rounds of
    // MakeMutations' recursion: tens to hundreds of edits per region) reads a few percent of them: the fills then run as strip
    // sweeps that keep those columns only (ps_sweep.hip, k_sweeps) — a few MB per alignment instead of 2 x 110 MB.  A list that
    // touches more than a quarter of the columns (Refine's point edits at every position) takes full matrices.
    static const double sparse_frac = getenv("PORESEQ_SPARSE_FRAC") ? atof(getenv("PORESEQ_SPARSE_FRAC")) : 0.25;
    bool sparse = sweep_enabled();
    int njobs_all = 0;
    double sparse_bytes = 0;
    for (int k = 0; k < R && sparse; k++) {
        const Align* a = as[k];
        const int C = (int)a->states.size();
        if (plan[k].keep[0].empty()) plan_keep(a, &plan[k]);   // (C + 2 entries once computed)
        if (std::max(plan[k].nkeep[0], plan[k].nkeep[1]) > sparse_frac * C) sparse = false;
        const int K = sweep_guess_k(a->par.realign_width);
        if (!K) sparse = false;
        njobs_all += a->E;
        for (int e = 0; e < a->E && sparse; e++)
            sparse_bytes += 1.15 * sweep_job_bytes(a->n[e], C, sweep_guess_form(a->par.realign_width, 1)) + 16.0 * (plan[k].nkeep[0] + plan[k].nkeep[1]) * (std::min(2 * a->par.realign_width + 1, a->n[e]) + 24);
    }
    if (sparse && 2 * njobs_all < sparse_min()) sparse = false;
    if (tk.on) {
        double fr = 0; size_t M = 0;
        for (int k = 0; k < R; k++) { M += plan[k].M; if (!plan[k].keep[0].empty()) fr = std::max(fr, (double)std::max(plan[k].nkeep[0], plan[k].nkeep[1]) / std::max<size_t>(as[k]->states.size(), 1)); }
        fprintf(stderr, "[ps] score_mutations: %d regions, %d events, %zu edits, kept columns <= %.3f of a matrix: %s\n", R, njobs_all, M, fr, sparse ? "kept columns" : "full matrices");
    }
    tk.lap("edit sizes");
    auto sub = [&](size_t k0, size_t k1) {   // regions k0 .. k1 - 1 as a call of their own, with their plans
        std::vector<double*> dsub;
        if (delta_out) dsub.assign(delta_out->begin() + k0, delta_out->begin() + k1);
        std::vector<EditPlan> psub(std::make_move_iterator(plan.begin() + k0), std::make_move_iterator(plan.begin() + k1));
        PointOut ptsub;
        if (pt) { ptsub.table.assign(pt->table.begin() + k0, pt->table.begin() + k1); ptsub.best.assign(pt->best.begin() + k0, pt->best.begin() + k1); }
        SupportOut spsub;
        if (sp) {
            spsub.group.assign(sp->group.begin() + k0, sp->group.begin() + k1); spsub.ngroups.assign(sp->ngroups.begin() + k0, sp->ngroups.begin() + k1);
            spsub.score.assign(sp->score.begin() + k0, sp->score.begin() + k1); spsub.rec.assign(sp->rec.begin() + k0, sp->rec.begin() + k1);
            spsub.geno = sp->geno;
            if (sp->geno) {
                spsub.nfrac.assign(sp->nfrac.begin() + k0, sp->nfrac.begin() + k1); spsub.frac.assign(sp->frac.begin() + k0, sp->frac.begin() + k1);
                spsub.lik.assign(sp->lik.begin() + k0, sp->lik.begin() + k1); spsub.ncover.assign(sp->ncover.begin() + k0, sp->ncover.begin() + k1);
            }
        }
        return score_mutations_planned(rt, std::vector<Align*>(as.begin() + k0, as.begin() + k1),
                                       std::vector<const std::vector<Mut>*>(muts.begin() + k0, muts.begin() + k1),
                                       pt || sp ? std::vector<std::vector<Mut>*>() : std::vector<std::vector<Mut>*>(outs.begin() + k0, outs.begin() + k1),
                                       delta_out ? &dsub : nullptr, psub, pt ? &ptsub : nullptr, sp ? &spsub : nullptr);
    };
    if (sparse && R > 1 && sparse_bytes > device_share_bytes()) return in_halves(as.size(), sub);
    if (!sparse && fit_share(as, 0, 2) < as.size()) return in_share_chunks(as, 2, sub);   // sub-batches that fit a slab
    // the kept-column tables of all AlignData in one block (before the jobs are built: their descriptors point into it)
    std::vector<const int*> d_keep(2 * (size_t)R, nullptr);
    if (sparse) {
        size_t tot = 0;
        for (int k = 0; k < R; k++) tot += plan[k].keep[0].size() + plan[k].keep[1].size();
        DBuf& kb = rt->buf("keep");
        PS_TRY(kb.ensure(std::max<size_t>(tot, 1) * sizeof(int)));
        std::vector<int> hk;
        hk.reserve(tot);
        for (int k = 0; k < R; k++)
            for (int d = 0; d < 2; d++) { d_keep[2 * k + d] = kb.as<int>() + hk.size(); hk.insert(hk.end(), plan[k].keep[d].begin(), plan[k].keep[d].end()); }
        PS_TRY(rt->up(kb.p, hk.data(), hk.size() * sizeof(int)));
    }
    // Alignment::update for every event of every AlignData: enqueued now, so that the fills run while the host prepares the edit tables
    std::vector<JobSpec> specs;
    std::vector<int> job0(R, 0);
    int extra = 0;
    for (int k = 0; k < R; k++) {
        Align* a = as[k];
        job0[k] = (int)specs.size();
        extra = std::max(extra, plan[k].extra);
        for (int e = 0; e < a->E; e++) {
            JobSpec s = a->job(e);
            if (sparse) for (int d = 0; d < 2; d++) { s.keep[d] = d_keep[2 * k + d]; s.nkeep[d] = plan[k].nkeep[d]; }
            specs.push_back(s);
        }
    }
    // the per-position layout of FindPointMutations' list (point_layout); an AlignData without events has every score at its seed,
    // -1e-6 (score_mutations): its rows are written here
    std::vector<std::vector<int>> pfirst(pt ? R : 0), ptriv(pt ? R : 0);
    if (pt)
        for (int k = 0; k < R; k++) {
            point_layout(as[k], &pfirst[k], &ptriv[k]);
            if (!as[k]->E) point_rows_seed(ptriv[k], pt->table[k], pt->best[k]);
        }
    // a support call: an AlignData without events has every score at its seed and all-zero records
    if (sp)
        for (int k = 0; k < R; k++)
            if (!as[k]->E) {
                if (sp->score[k]) std::fill(sp->score[k], sp->score[k] + plan[k].M, -1e-6);
                if (sp->rec[k]) memset(sp->rec[k], 0, (size_t)plan[k].M * sp->ngroups[k] * sizeof(ps_edit_support));
                if (sp->geno) {   // (and no covering event: all-zero likelihoods)
                    std::fill(sp->lik[k], sp->lik[k] + (size_t)plan[k].M * (sp->nfrac[k] + 1), 0.0);
                    if (sp->ncover[k]) std::fill(sp->ncover[k], sp->ncover[k] + plan[k].M, 0);
                }
            }
    if (specs.empty()) return PS_OK;
    Batch b;
    SlabHold slab;   // full matrices: one of the process's slabs for the duration of this call (released at every return)
    double lone_need = 0;   // a single AlignData cannot be split: matrices beyond a slab go to the runtime's own pools
    if (!sparse && R == 1) for (int e = 0; e < as[0]->E; e++) lone_need += matrix_bytes((int64_t)as[0]->n[e] + (int64_t)as[0]->states.size() + 1, most_slots_w(as[0]->par.realign_width), 2);
    if (!sparse && lone_need <= (double)slab_bytes()) {
        PS_TRY(slab_acquire(&slab));
        if (R == 1 && lone_need > (double)slab.bytes) {
            // the slab this call was handed is smaller than the plan (a device fuller than expected: slab_acquire's fallback sizes) and a
            // single AlignData cannot be split: its matrices go to the runtime's own pools, as those beyond a planned slab do
            slab.release();
        } else {
            if (rt->prof_on) rt->prof["slab"].launches++;   // (dense calls that took a slab: a host-side count)
            slab.drain = rt->stream;
            b.ext = slab.p; b.ext_bytes = R > 1 ? std::min(slab.bytes, (size_t)dense_cap_bytes()) : slab.bytes;
        }
        tk.lap("slab wait");
    }
    PS_TRY(b.build(rt, specs, 2, extra));
    {
        const int rc = realign(rt, b, R > 1 ? (sparse ? PLAN_OVER_GUESS * device_share_bytes() : (double)b.ext_bytes) : 0.0);
        if (rc == PS_SPLIT) { slab.release(); return in_halves(as.size(), sub); }   // bands wider than guessed: two halves, one after the other
        PS_TRY(rc);
    }
    for (Align* a : as) a->host_refs_valid = false;
    tk.lap("realign enqueue");
    par_for(R, [&](int k) { plan_tables(as[k], *muts[k], &plan[k], R == 1 ? 8 : (R <= 4 ? 4 : 1)); });
    tk.lap("edit geometry");
    // upload the edit tables of all AlignData in one block
    size_t ints = 16, dbls = 1;
    for (int k = 0; k < R; k++) {
        const EditPlan& p = plan[k];
        ints += (size_t)p.M * 7 + (size_t)p.M * p.ncolmax + p.nr0 + 16;
        if (pt) ints += pfirst[k].size() + ptriv[k].size();
        if (sp) ints += (size_t)as[k]->E;
        dbls += (size_t)as[k]->E * std::max(p.nr0, 1) + (size_t)as[k]->E * std::max(p.M, 1) + std::max(p.M, 1) + (size_t)as[k]->E * (as[k]->states.size() + 8);
    }
    DBuf& mb = rt->buf("mutint");
    PS_TRY(mb.ensure(ints * sizeof(int) + 128 + (size_t)R * (sizeof(ScoreArgs) + std::max(sizeof(PointArgs), sizeof(SupportArgs)) + sizeof(GenoArgs)) + 64));
    DBuf& db = rt->buf("mutdbl");
    PS_TRY(db.ensure(dbls * sizeof(double)));
    int* dp = mb.as<int>();
    double* dd = db.as<double>();
    // every AlignData's score array first, back to back: ONE device-to-host copy returns them all (a copy per region before:
    // 20 000 of a bench step's 25 000 copy commands, ~0.2 ms each on a loaded stream)
    double* const score0 = dd;
    size_t score_tot = 0;
    std::vector<size_t> score_at(R, 0);
    for (int k = 0; k < R; k++) { score_at[k] = score_tot; score_tot += (size_t)std::max(plan[k].M, 1); }
    dd += score_tot;
    std::vector<int> stage;
    stage.reserve(ints);
    auto push = [&](const std::vector<int>& v) { int* r = dp + stage.size(); stage.insert(stage.end(), v.begin(), v.end()); return r; };
    // a point-table call: the records, then the rows, of all AlignData back to back in one buffer — ONE device-to-host copy
    std::vector<size_t> best_at(R, 0), table_at(R, 0);
    size_t pt_bytes = 0;
    char* d_pt = nullptr;
    if (pt) {
        for (int k = 0; k < R; k++) if (pt->best[k] && as[k]->E) { best_at[k] = pt_bytes; pt_bytes += ptriv[k].size() * sizeof(ps_point_best); }
        for (int k = 0; k < R; k++) if (pt->table[k] && as[k]->E) { table_at[k] = pt_bytes; pt_bytes += ptriv[k].size() * PT_SLOTS * sizeof(double); }
        DBuf& pb = rt->buf("ptable");
        PS_TRY(pb.ensure(std::max<size_t>(pt_bytes, 16)));
        d_pt = pb.as<char>();
    }
    // a support call: the scores, then the records, of all AlignData back to back in one buffer — ONE device-to-host copy; a genotype
    // call's likelihoods and covering-event counts follow them in the same buffer and come back in the same copy
    std::vector<size_t> sscore_at(R, 0), srec_at(R, 0), glik_at(R, 0), gcov_at(R, 0);
    size_t sp_bytes = 0;
    char* d_sp = nullptr;
    auto sp_live = [&](int k) { return plan[k].M > 0 && as[k]->E > 0; };
    if (sp) {
        for (int k = 0; k < R; k++) if (sp_live(k)) { sscore_at[k] = sp_bytes; sp_bytes += (size_t)plan[k].M * sizeof(double); }
        for (int k = 0; k < R; k++) if (sp_live(k) && sp->rec[k]) { srec_at[k] = sp_bytes; sp_bytes += (size_t)plan[k].M * sp->ngroups[k] * sizeof(ps_edit_support); }
        if (sp->geno) {
            for (int k = 0; k < R; k++) if (sp_live(k)) { glik_at[k] = sp_bytes; sp_bytes += (size_t)plan[k].M * (sp->nfrac[k] + 1) * sizeof(double); }
            for (int k = 0; k < R; k++) if (sp_live(k)) { gcov_at[k] = sp_bytes; sp_bytes += (size_t)plan[k].M * sizeof(int32_t); }
        }
        DBuf& sb = rt->buf("support");
        PS_TRY(sb.ensure(std::max<size_t>(sp_bytes, 16)));
        d_sp = sb.as<char>();
    }
    std::vector<ScoreArgs> sas(R);
    std::vector<PointArgs> pts(pt ? R : 0);
    std::vector<SupportArgs> sps(sp ? R : 0);
    std::vector<GenoArgs> gts(sp && sp->geno ? R : 0);
    for (int k = 0; k < R; k++) {
        const EditPlan& p = plan[k];
        ScoreArgs& sa = sas[k];
        memset(&sa, 0, sizeof(sa));
        sa.job0 = job0[k]; sa.njobs = as[k]->E;
        sa.nitems_per_job = p.M; sa.ncolmax = p.ncolmax; sa.ws = as[k]->par.scoring_width; sa.nr0 = p.nr0;
        sa.m_start = push(p.start); sa.m_mlen = push(p.mlen); sa.m_cm = push(p.cm); sa.m_ncol = push(p.ncol);
        sa.m_skip = push(p.skip); sa.m_oldidx = push(p.oldidx); sa.m_states = push(p.states); sa.r0 = push(p.r0s);
        for (int q = 0; q < SCORE_CLASSES; q++) { sa.cls_items[q] = push(p.cls[q]); sa.cls_count[q] = (int)p.cls[q].size(); }
        sa.old = dd; dd += (size_t)as[k]->E * std::max(p.nr0, 1);
        sa.delta = dd; dd += (size_t)as[k]->E * std::max(p.M, 1);
        sa.score = score0 + score_at[k];
        // edit positions on more than a quarter of the columns: column-pair maxima of ALL columns in one coalesced pass (k_oldall)
        sa.oldall_pitch = (int64_t)as[k]->states.size() + 8;
        sa.maxS = b.maxS;
        sa.oldall = !b.sparse && (size_t)p.nr0 * 4 > as[k]->states.size() && p.nr0 >= 256 ? dd : nullptr;   // (k_oldall walks full matrices)
        if (sa.oldall) PS_HIP(hipMemsetAsync(sa.oldall, 0, (size_t)as[k]->E * sa.oldall_pitch * sizeof(double), rt->stream));
        dd += (size_t)as[k]->E * sa.oldall_pitch;
        if (pt) {
            PointArgs& q = pts[k];
            memset(&q, 0, sizeof(q));
            q.pos_first = push(pfirst[k]); q.pos_triv = push(ptriv[k]); q.npos = (int)ptriv[k].size();
            if (pt->table[k] && as[k]->E) q.table = (double*)(d_pt + table_at[k]);
            if (pt->best[k] && as[k]->E) q.best = (ps_point_best*)(d_pt + best_at[k]);
            if (!q.table && !q.best) q.npos = 0;
        }
        if (sp) {
            SupportArgs& q = sps[k];
            memset(&q, 0, sizeof(q));
            q.group = push(std::vector<int>(sp->group[k], sp->group[k] + as[k]->E));
            if (sp_live(k) && sp->rec[k]) { q.ngroups = sp->ngroups[k]; q.score = (double*)(d_sp + sscore_at[k]); q.out = (ps_edit_support*)(d_sp + srec_at[k]); }
        }
        if (sp && sp->geno) {
            GenoArgs& q = gts[k];
            memset(&q, 0, sizeof(q));
            q.nfrac = -1;
            if (sp_live(k)) {
                q.nfrac = sp->nfrac[k];
                for (int i = 0; i < q.nfrac; i++) { q.f[i] = sp->frac[k][i]; q.g[i] = 1.0 - q.f[i]; }
                if (!sp->rec[k]) q.score = (double*)(d_sp + sscore_at[k]);   // (k_support writes nothing for this AlignData)
                q.lik = (double*)(d_sp + glik_at[k]); q.ncover = (int*)(d_sp + gcov_at[k]);
            }
        }
        if (!p.M || !as[k]->E) { sa.njobs = 0; sa.nitems_per_job = 0; }   // nothing to score for this AlignData: its blocks leave at once
    }
    // the edit tables and their descriptors (ScoreArgs, behind the tables in the same buffer) in one copy
    const size_t sa_at = (stage.size() * sizeof(int) + 63) / 64 * 64;
    const size_t pt_at = (sa_at + (size_t)R * sizeof(ScoreArgs) + 63) / 64 * 64;   // (a point-table call: its PointArgs behind them)
    const size_t gt_at = (pt_at + sps.size() * sizeof(SupportArgs) + 63) / 64 * 64;                       // (a genotype call: its GenoArgs behind the SupportArgs)
    std::vector<char> blob(std::max(pt_at + pts.size() * sizeof(PointArgs), gt_at + gts.size() * sizeof(GenoArgs)));   // (PointArgs or SupportArgs, never both)
    memcpy(blob.data(), stage.data(), stage.size() * sizeof(int));
    memcpy(blob.data() + sa_at, sas.data(), (size_t)R * sizeof(ScoreArgs));
    if (pt) memcpy(blob.data() + pt_at, pts.data(), pts.size() * sizeof(PointArgs));
    if (sp) memcpy(blob.data() + pt_at, sps.data(), sps.size() * sizeof(SupportArgs));
    if (!gts.empty()) memcpy(blob.data() + gt_at, gts.data(), gts.size() * sizeof(GenoArgs));
    PS_TRY(rt->up(dp, blob.data(), blob.size()));
    const ScoreArgs* d_sas = (const ScoreArgs*)((const char*)dp + sa_at);
    const PointArgs* d_pts = pt ? (const PointArgs*)((const char*)dp + pt_at) : nullptr;
    const SupportArgs* d_sps = sp ? (const SupportArgs*)((const char*)dp + pt_at) : nullptr;
    const GenoArgs* d_gts = !gts.empty() ? (const GenoArgs*)((const char*)dp + gt_at) : nullptr;
    tk.lap("upload");
    if (tk.on) { PS_HIP(hipStreamSynchronize(rt->stream)); }
    tk.lap("realign fwd+back (rest)");
    PS_TRY(launch_lb(rt, b.d, 1, b.maxlbn));
    std::vector<double*> sc(R, nullptr);
    for (int k = 0; k < R; k++) {
        const EditPlan& p = plan[k];
        if (!p.M || !as[k]->E) continue;
        if (rt->prof_on) {
            // per (event, edit) item  16(Bs+1) + 16 Br + 24(Bs+c) + 32 Br / k + 8
            double t = 0;
            const double Bs = 2.0 * sas[k].ws + 1, Br = 2.0 * as[k]->par.realign_width + 1;
            const double kk = (double)p.M / std::max(p.nr0, 1);
            for (int i = 0; i < p.M; i++) t += 16 * (Bs + 1) + 16 * Br + 24 * (Bs + p.mlen[i] + 6) + 32 * Br / kk + 8;
            rt->prof["score"].bytes += t * as[k]->E;
            rt->prof["score"].units += (double)p.M * as[k]->E;
        }
    }
    PS_TRY(launch_score(rt, b.d, d_sas, sas, d_pts, pt ? &pts : nullptr, d_sps, sp ? &sps : nullptr, d_gts, d_gts ? &gts : nullptr));
    if (sp) {
        char* h_sp = nullptr;
        if (sp_bytes) PS_TRY(rt->down((void**)&h_sp, d_sp, sp_bytes));
        PS_HIP(hipStreamSynchronize(rt->stream));
        for (int k = 0; k < R; k++) {
            if (!sp_live(k)) continue;
            if (sp->score[k]) memcpy(sp->score[k], h_sp + sscore_at[k], (size_t)plan[k].M * sizeof(double));
            if (sp->rec[k]) memcpy(sp->rec[k], h_sp + srec_at[k], (size_t)plan[k].M * sp->ngroups[k] * sizeof(ps_edit_support));
            if (sp->geno) {
                memcpy(sp->lik[k], h_sp + glik_at[k], (size_t)plan[k].M * (sp->nfrac[k] + 1) * sizeof(double));
                if (sp->ncover[k]) memcpy(sp->ncover[k], h_sp + gcov_at[k], (size_t)plan[k].M * sizeof(int32_t));
            }
        }
        tk.lap("score edits");
        return PS_OK;
    }
    if (pt) {
        char* h_pt = nullptr;
        if (pt_bytes) PS_TRY(rt->down((void**)&h_pt, d_pt, pt_bytes));
        PS_HIP(hipStreamSynchronize(rt->stream));
        for (int k = 0; k < R; k++) {
            if (!as[k]->E || ptriv[k].empty()) continue;
            if (pt->best[k]) memcpy(pt->best[k], h_pt + best_at[k], ptriv[k].size() * sizeof(ps_point_best));
            if (pt->table[k]) memcpy(pt->table[k], h_pt + table_at[k], ptriv[k].size() * PT_SLOTS * sizeof(double));
        }
        tk.lap("score edits");
        return PS_OK;
    }
    std::vector<double*> dl(R, nullptr);
    double* all_scores = nullptr;
    PS_TRY(rt->down(&all_scores, score0, score_tot));
    for (int k = 0; k < R; k++)
        if (plan[k].M && as[k]->E) {
            sc[k] = all_scores + score_at[k];
            if (delta_out && (*delta_out)[k]) PS_TRY(rt->down(&dl[k], sas[k].delta, (size_t)as[k]->E * plan[k].M));
        }
    PS_HIP(hipStreamSynchronize(rt->stream));
    for (int k = 0; k < R; k++) {
        if (sc[k]) for (int i = 0; i < plan[k].M; i++) (*outs[k])[i].score = sc[k][i];
        if (dl[k]) memcpy((*delta_out)[k], dl[k], (size_t)as[k]->E * plan[k].M * sizeof(double));
    }
    tk.lap("score edits");
    return PS_OK;
}

// ScorePoints (ScoreMutations on FindPointMutations' list, at the scoring width the AlignData carries) for several AlignData, reduced on
// the device to a row per position (k_point_table) instead of a scored list: the same chain as score_mutations_multi up to k_score,
// then one copy back of all rows and records.  tables[k]: null or [states][9]; bests[k]: null or [states].
int point_table_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<double*>& tables, const std::vector<ps_point_best*>& bests) {
    const int R = (int)as.size();
    std::vector<std::vector<Mut>> lists(R);
    std::vector<EditPlan> plan(R);
    std::vector<const std::vector<Mut>*> muts(R);
    par_for(R, [&](int k) {
        find_point_mutations(as[k], &lists[k]);
        plan_edits(as[k], lists[k], &plan[k]);
        muts[k] = &lists[k];
    });
    for (int k = 0; k < R; k++) {
        if (as[k]->par.scoring_width < 0) return fail(PS_ERR_BAD_ARG, "scoring_width < 0");
        if (plan[k].rc != PS_OK) return fail(plan[k].rc, "negative mutation start");
    }
    PointOut pt;
    pt.table = tables; pt.best = bests;
    return score_mutations_planned(rt, as, muts, {}, nullptr, plan, &pt);
}

// ps_score_mutation_support / ps_batch_score_mutation_support: the chain of score_mutations_multi up to k_score, then k_support instead
// of k_reduce and one copy back of all scores and records.  group[k]: [E] ids in 0 .. ngroups[k] - 1 (checked by the caller);
// scores[k]: null or [M]; recs[k]: [M][ngroups[k]].
int score_mutation_support_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<Mut>*>& muts,
                                 const std::vector<const int32_t*>& group, const std::vector<int>& ngroups,
                                 const std::vector<double*>& scores, const std::vector<ps_edit_support*>& recs) {
    const int R = (int)as.size();
    std::vector<EditPlan> plan(R);
    par_for(R, [&](int k) { plan_edits(as[k], *muts[k], &plan[k]); });
    for (int k = 0; k < R; k++) {
        if (as[k]->par.scoring_width < 0) return fail(PS_ERR_BAD_ARG, "scoring_width < 0");
        if (plan[k].rc != PS_OK) return fail(plan[k].rc, "negative mutation start");
        if (plan[k].ncolmax > 64 && as[k]->par.scoring_width > 511) return fail(PS_ERR_UNSUPPORTED, "edit longer than 58 bases with scoring_width > 511");
    }
    SupportOut sp;
    sp.group = group; sp.ngroups = ngroups; sp.score = scores; sp.rec = recs;
    return score_mutations_planned(rt, as, muts, {}, nullptr, plan, nullptr, &sp);
}

// ps_score_mutation_genotypes / ps_batch_score_mutation_genotypes: score_mutation_support_multi with k_genotype behind k_support, and the
// likelihoods and covering-event counts in the same copy back.  recs[k] and ncover[k] may be null; frac[k]: [nfrac[k]] alt fractions
// (checked by the caller); lik[k]: [M][nfrac[k] + 1].
int score_mutation_genotypes_multi(Runtime* rt, const std::vector<Align*>& as, const std::vector<const std::vector<Mut>*>& muts,
                                   const std::vector<const int32_t*>& group, const std::vector<int>& ngroups,
                                   const std::vector<int>& nfrac, const std::vector<const double*>& frac,
                                   const std::vector<double*>& scores, const std::vector<ps_edit_support*>& recs,
                                   const std::vector<double*>& lik, const std::vector<int32_t*>& ncover) {
    const int R = (int)as.size();
    std::vector<EditPlan> plan(R);
    par_for(R, [&](int k) { plan_edits(as[k], *muts[k], &plan[k]); });
    for (int k = 0; k < R; k++) {
        if (as[k]->par.scoring_width < 0) return fail(PS_ERR_BAD_ARG, "scoring_width < 0");
        if (plan[k].rc != PS_OK) return fail(plan[k].rc, "negative mutation start");
        if (plan[k].ncolmax > 64 && as[k]->par.scoring_width > 511) return fail(PS_ERR_UNSUPPORTED, "edit longer than 58 bases with scoring_width > 511");
    }
    SupportOut sp;
    sp.group = group; sp.ngroups = ngroups; sp.score = scores; sp.rec = recs;
    sp.geno = true; sp.nfrac = nfrac; sp.frac = frac; sp.lik = lik; sp.ncover = ncover;
    return score_mutations_planned(rt, as, muts, {}, nullptr, plan, nullptr, &sp);
}

int score_mutations(Runtime* rt, Align* a, const std::vector<Mut>& muts, std::vector<Mut>* out) {
    if (!a->E) {
        *out = muts;
        for (Mut& m : *out) m.score = -1e-6;
        for (const Mut& m : muts) if (m.start < 0) return fail(PS_ERR_BAD_ARG, "negative mutation start");
        return PS_OK;
    }
    return score_mutations_multi(rt, {a}, {&muts}, {out});
}

// FindPointMutations, cpp/FindMutations.cpp:191-234
void find_point_mutations(const Align* a, std::vector<Mut>* out) {
    static const char B4[] = "ACGT";
    out->clear();
    out->reserve(a->states.size() * 8);
    for (size_t i = 0; i < a->states.size(); i++) {
        Mut m;
        m.start = (int)i;
        m.orig.assign(1, a->bases[i]);
        out->push_back(m);
        for (int k = 0; k < 4; k++) {
            if (a->bases[i] == B4[k]) continue;
            m.mut.assign(1, B4[k]);
            out->push_back(m);
        }
        m.orig.clear();
        for (int k = 0; k < 4; k++) { m.mut.assign(1, B4[k]); out->push_back(m); }
    }
    if (a->par.verbose) { fputs("Point ", stderr); fflush(stderr); }   // cpp/FindMutations.cpp:230-231
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
        std::vector<Align*> sa;
        std::vector<const std::vector<Mut>*> in;
        std::vector<std::vector<Mut>*> out;
        for (int k : next) { sa.push_back(as[k]); in.push_back(&later[k]); out.push_back(&muts[k]); }
        PS_TRY(score_mutations_multi(rt, sa, in, out));
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
