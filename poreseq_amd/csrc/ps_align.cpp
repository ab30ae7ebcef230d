// ps_align.cpp — struct Align (ps_host.h): an AlignData (cpp/AlignData.h:26-35) with its event data resident in HBM.  create()
// marshals the events into one slab (ps_mem.cpp's cache) and decides with ps_sane.h which emissions are refused, marked or safe
// for tabulated reciprocals; job() / base_batch() describe its events to a Batch (ps_host.cpp); the refs_* functions mirror
// ref_align / ref_like to the host; keep_refs / restore_refs are ps_align_keep_refs / ps_align_new_call.
#include "ps_host.h"
#include "ps_sane.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ps {
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

}  // namespace ps
