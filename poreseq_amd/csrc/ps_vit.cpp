// ps_vit.cpp — the host chain of ViterbiMutate (cpp/Viterbi.cpp:239-426) for several AlignData in lock-step.  One call record and one
// request record per AlignData (VitCall, VitReq, ps_host.h) and one chain, viterbi_mutate: the checks, the refs to the host, the
// walk over the reference positions (vit_gather, ps_vitgather.h), the cut into sub-batches that fit this runtime's share, each
// sub-batch through viterbi_batch — plan, place, upload, emissions, steps, tap, draw, the deterministic (vit_follow_bp,
// ps_vitpath.h) or the stochastic tail — and the paths to bases.  The kernels and their launchers are ps_viterbi.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ps_host.h"
#include "ps_vitgather.h"
#include "ps_vitpath.h"

namespace ps {

inline int succ(int st, int k, int j) { return ((st << (2 * j)) & (NS - 1)) + k; }   // cpp/Viterbi.h:31-32
inline char base_at(int st, int k) { return "ACGT"[3 & (st >> (2 * (4 - k)))]; }    // cpp/Viterbi.h:35-39

// StatesToSequence, cpp/Viterbi.cpp:171-237
static std::string path_to_bases(const int16_t* st, size_t len) {
    std::string s;
    int cur = st[0];
    s.push_back(base_at(cur, 0));
    for (size_t i = 1; i < len; i++) {
        if (cur == st[i]) continue;
        bool hit = false;
        for (int n = 1; n <= 4 && !hit; n++)
            for (int k = 0; k < (1 << (2 * n)); k++)
                if (succ(cur, k, n) == st[i]) {
                    for (int b = 1; b <= n; b++) s.push_back(base_at(cur, b));
                    cur = st[i]; hit = true; break;
                }
        if (!hit) { cur = st[i]; s.push_back(base_at(cur, 0)); }
    }
    for (int b = 1; b <= 4; b++) s.push_back(base_at(cur, b));
    return s;
}

// rand() of a fresh process, per region: glibc's reentrant random_r() on a 128-byte TYPE_3 state is the generator behind
// rand() minus the process-wide lock.  A state is either the calling thread's (ps_srand / ps_rand_draw, the single-handle
// ABI) or an explicit ps_rng object that a lock-step driver keeps per region (include/poreseq_hip.h).
struct RandState {
    random_data rd;
    char st[128];
    bool init = false;
};
namespace { thread_local RandState t_rand; }
static void rs_seed(RandState* r, unsigned seed) {
    memset(&r->rd, 0, sizeof(r->rd));
    initstate_r(seed, r->st, sizeof(r->st), &r->rd);
    r->init = true;
}
static int rs_next(RandState* r) {
    if (!r->init) rs_seed(r, 1);
    int32_t v = 0;
    random_r(&r->rd, &v);
    return (int)v;
}
void rand_seed(unsigned seed) { rs_seed(&t_rand, seed); }
int rand_next() { return rs_next(&t_rand); }
RandState* rand_state_new(unsigned seed) { RandState* r = new RandState(); rs_seed(r, seed); return r; }
void rand_state_free(RandState* r) { delete r; }
void rand_state_seed(RandState* r, unsigned seed) { rs_seed(r, seed); }
int rand_state_next(RandState* r) { return rs_next(r ? r : &t_rand); }

// uniform deviates in the reference's call order: for each kept path, one per back-step (cpp/Viterbi.cpp:108)
static void vit_draw(void* rng, double* rnd, size_t n) {
    RandState* r = (RandState*)rng;
    for (size_t k = 0; k < n; k++) rnd[k] = rand_state_next(r) / (double(RAND_MAX) + 1);
}

namespace {
// One call on its way through the stages below, which fill it in this order
struct Vit {
    Runtime* rt;
    const VitCall& call;
    VitReq* reqs;
    int R;
    Tick tk;
    std::vector<double*> h_ri;       // per AlignData: host mirrors of ref_index and of the events' JobOut records
    std::vector<JobOut*> info;
    std::vector<VitGather> gath;     // per AlignData: the kept positions and their levels
    std::vector<VitRegionH> regs;    // per AlignData: the record the sub-batches run on; its paths come back in it
    Vit(Runtime* rt_, const VitCall& call_, VitReq* reqs_, size_t n) : rt(rt_), call(call_), reqs(reqs_), R((int)n), tk("viterbi_mutate") {}
    std::string named(int r) const { return std::string(call.who) + ": " + (call.lockstep ? "region " + std::to_string(r) + ": " : std::string()); }
};
}  // namespace

// ---- stage: checks, before a runtime is asked for.  A single-handle entry answers with its bare name.  Emissions that are
// -infinity or NaN: a position whose candidates are all NaN leaves the back-pointer -1 behind (k_vit_steps), which the back-trace
// would index with — refused
static int check_call(const VitCall& c, const VitReq* reqs, size_t n) {
    const std::string who(c.who);
    if (c.nkeep < 0) return fail(PS_ERR_BAD_ARG, c.lockstep ? who + ": nkeep" : who);
    for (size_t k = 0; k < n; k++) if (reqs[k].a->E == 0) return fail(PS_ERR_BAD_ARG, c.lockstep ? who + ": no events" : who);
    for (size_t k = 0; k < n; k++) {
        const Align& a = *reqs[k].a;
        if (!a.nonfinite.empty())
            return fail(PS_ERR_BAD_ARG, who + ": " + a.nonfinite + " (ViterbiMutate needs finite levels with stdv > 0 and a model with positive deviations)");
    }
    return PS_OK;
}

// ---- stage: refs to host.  Mirrors of ref_align / ref_index / refstart / refend, one synchronisation for all
static int refs_to_host(Vit& v) {
    v.h_ri.assign(v.R, nullptr);
    v.info.assign(v.R, nullptr);
    for (int r = 0; r < v.R; r++) {
        Align* a = v.reqs[r].a;
        PS_TRY(a->refs_to_host_async(v.rt));
        a->last_stream = (void*)v.rt->stream;   // (the copies here, and the Viterbi kernels read the model tables in the AlignData's slab)
        PS_TRY(v.rt->down(&v.h_ri[r], a->d_ri, (size_t)a->ntot));
        PS_TRY(v.rt->down(&v.info[r], a->d_out, (size_t)a->E));
    }
    PS_HIP(hipStreamSynchronize(v.rt->stream));
    for (int r = 0; r < v.R; r++) v.reqs[r].a->refs_finish();
    v.tk.lap("refs D2H");
    return PS_OK;
}

// ---- stage: checks on the host copy, before any kernel of the call.  The walk runs from the smallest refstart to the largest refend,
// both (int)ref_align of an aligned level (cpp/EventData.h:135-136): an entry that is not below 2^31, +inf included, has no defined
// conversion and would send vit_gather towards 2^31 — refused, naming the event and the level.  The DP and the census take any
// double (include/poreseq_hip.h).
static int check_refs(const Vit& v) {
    for (int r = 0; r < v.R; r++) {
        const Align& a = *v.reqs[r].a;
        for (int e = 0; e < a.E; e++) {
            const double* ra = a.h_ra.data() + a.off[e];
            for (int t = 0; t < a.n[e]; t++)
                if (ra[t] >= 2147483648.0) {
                    char val[64];
                    snprintf(val, sizeof(val), "%g", ra[t]);
                    return fail(PS_ERR_BAD_ARG, v.named(r) + "event " + std::to_string(e) + ", level " + std::to_string(t) + ": ref_align = " + val +
                                                    " is not below 2^31 (ViterbiMutate walks the positions from (int)ref_align)");
                }
        }
    }
    return PS_OK;
}

// ---- stage: gather.  Which reference positions are kept and the mean level per (position, event), per AlignData on host threads;
// then the records the sub-batches run on
static void gather(Vit& v) {
    v.gath.resize(v.R);
    par_for(v.R, [&](int r) {
        const Align* a = v.reqs[r].a;
        std::vector<VitGatherEvent> ev(a->E);
        for (int e = 0; e < a->E; e++) ev[e] = {a->n[e], a->off[e], v.info[r][e].has_index != 0, v.info[r][e].refstart, v.info[r][e].refend};
        vit_gather({a->E, ev.data(), a->h_ra.data(), v.h_ri[r], a->h_mean.data(), a->h_stdv.data()}, &v.gath[r]);
    });
    v.tk.lap("gather levels");
    v.regs.resize(v.R);
    for (int r = 0; r < v.R; r++) {
        VitRegionH& g = v.regs[r];
        g.E = v.reqs[r].a->E; g.T = v.gath[r].T; g.obsin = v.gath[r].obsin.data(); g.d_model = v.reqs[r].a->d_model;
        g.rng = v.reqs[r].rng; g.draw = vit_draw;
        g.index = v.call.lockstep ? r : -1;
    }
}

// ---- stage: cut.  Sub-batches of regions that fit this runtime's device share (obs, trimmed means, back-pointers and forward
// probabilities: 26 KB per position; ~270 MB per 10 kb region; the tables live in the runtime's matrix pool, which no alignment
// uses during this call); the regions' generators keep the results the same however the batch is cut; a sub-batch the device
// has no memory for is cut in two (nothing of it has been drawn yet: allocation comes first)
static int in_sub_batches(Vit& v) {
    auto need = [&](size_t k) { return 26.0 * 1024.0 * (double)v.regs[k].T + 32.0 * (double)v.regs[k].T * v.regs[k].E; };
    double cap = std::max(PLAN_VITERBI_FLOOR, PLAN_VITERBI_FRAC * device_share_bytes());
    for (size_t k0 = 0; k0 < v.regs.size();) {
        const size_t k1 = greedy_cut(k0, v.regs.size(), cap, (size_t)-1, need);
        const int rc = viterbi_batch(v.rt, v.call, v.regs.data() + k0, k1 - k0);
        if (rc == PS_ERR_NOMEM && k1 - k0 > 1) { cap *= 0.5; continue; }
        PS_TRY(rc);
        k0 = k1;
    }
    v.tk.lap("device");
    return PS_OK;
}

// ---- stage: paths to bases
static void to_bases(Vit& v) {
    par_for(v.R, [&](int r) {
        const VitRegionH& g = v.regs[r];
        for (size_t at = 0; at < g.paths.size(); at += (size_t)g.T) v.reqs[r].out->push_back(path_to_bases(g.paths.data() + at, (size_t)g.T));
    });
    v.tk.lap("paths to bases");
}

int viterbi_mutate(Runtime* rt, const VitCall& call, VitReq* reqs, size_t n) {
    PS_TRY(check_call(call, reqs, n));
    if (!rt) PS_TRY(runtime(&rt));
    Vit v(rt, call, reqs, n);
    for (int r = 0; r < v.R; r++) reqs[r].out->clear();
    PS_TRY(refs_to_host(v));
    PS_TRY(check_refs(v));
    gather(v);
    PS_TRY(in_sub_batches(v));
    to_bases(v);
    return PS_OK;
}

// ---------------------------------------------------------------------------------------------
// One sub-batch on the device.  The position x state tables (8 KB per position and table: 5.3 GB for 20 regions of 10 kb) live in
// the score-matrix pool: no alignment is in flight during a ViterbiMutate call, and a runtime that kept them beside the matrices
// would hold ~2 % of an MI355X for a phase that is 4 % of a schedule (seven runtimes: 38 GB that the matrices of the other phases
// can use).
namespace {
struct VitBatch {
    Runtime* rt;
    const VitCall& call;
    VitRegionH* regions;
    int R;
    VitTap* tap;
    // plan: the regions as the kernels see them, the region of every position, totals and the byte sizes of the arena's tables
    std::vector<VitReg> regs;
    std::vector<int> pos_reg;
    int64_t ttot = 0, intot = 0;
    int maxE = 0;
    size_t b_obs = 0, b_fwd = 0, b_bp = 0;
    // place
    VitReg* d_regs = nullptr;
    int* d_posreg = nullptr;
    double *d_in = nullptr, *d_obs = nullptr, *d_eobs = nullptr, *d_fwd = nullptr, *d_lik = nullptr;
    short* d_bp = nullptr;
    // steps, tap, draw: what is on its way to the host, the deviates, the start state of every region
    double *lik = nullptr, *tap_obs = nullptr, *tap_fwd = nullptr, *h_rand = nullptr;
    short* tap_bp = nullptr;
    std::vector<int> starts;
    VitBatch(Runtime* rt_, const VitCall& call_, VitRegionH* regions_, size_t n) : rt(rt_), call(call_), regions(regions_), R((int)n), tap(call_.tap) {}
    size_t cells() const { return (size_t)ttot * NS; }
};
}  // namespace

// ---- stage: plan.  Offsets and byte sizes; a tap gets its rows for the sub-batch's regions
static void plan(VitBatch& b) {
    b.regs.resize(b.R);
    for (int r = 0; r < b.R; r++) {
        const VitRegionH& g = b.regions[r];
        b.regions[r].paths.clear();
        b.regs[r].model = g.d_model; b.regs[r].E = g.E; b.regs[r].T = g.T;
        b.regs[r].in_off = b.intot; b.regs[r].t_off = b.ttot;
        b.intot += (int64_t)g.T * g.E * 4; b.ttot += g.T;
        b.maxE = std::max(b.maxE, g.E);
    }
    if (b.tap)
        for (int r = 0; r < b.R; r++) { b.tap->T.push_back(b.regions[r].T); b.tap->paths.emplace_back(); b.tap->lik_final.insert(b.tap->lik_final.end(), NS, 0.0); }
    if (b.ttot <= 0) return;
    b.pos_reg.resize((size_t)b.ttot);
    for (int r = 0; r < b.R; r++) std::fill(b.pos_reg.begin() + b.regs[r].t_off, b.pos_reg.begin() + b.regs[r].t_off + b.regs[r].T, r);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    b.b_obs = al(b.cells() * sizeof(double));
    b.b_fwd = al((size_t)(b.call.nkeep ? b.ttot : 1) * NS * sizeof(double));
    b.b_bp = al(b.cells() * sizeof(short));
}

// ---- stage: place.  Every allocation of the sub-batch before the first deviate is drawn: the caller may cut the batch again on PS_ERR_NOMEM
static int place(VitBatch& b) {
    Runtime* rt = b.rt;
    const int nkeep = b.call.nkeep;
    PS_TRY(rt->buf("vit_regs").ensure(b.R * sizeof(VitReg)));
    PS_TRY(rt->buf("vit_posreg").ensure((size_t)b.ttot * sizeof(int)));
    PS_TRY(rt->buf("vit_in").ensure((size_t)std::max<int64_t>(b.intot, 1) * sizeof(double)));
    DBuf& arena = rt->buf("rec");
    PS_TRY(arena.ensure(2 * b.b_obs + b.b_fwd + b.b_bp));
    PS_TRY(rt->buf("vit_lik").ensure((size_t)b.R * NS * sizeof(double)));
    if (nkeep > 0) {
        PS_TRY(rt->buf("vit_att").ensure(nkeep * sizeof(double)));
        PS_TRY(rt->buf("vit_start").ensure(b.R * sizeof(int)));
        PS_TRY(rt->buf("vit_rnd").ensure((size_t)nkeep * b.ttot * sizeof(double)));
        PS_TRY(rt->buf("vit_path").ensure((size_t)nkeep * b.ttot * sizeof(short)));
    }
    b.d_regs = rt->buf("vit_regs").as<VitReg>();
    b.d_posreg = rt->buf("vit_posreg").as<int>();
    b.d_in = rt->buf("vit_in").as<double>();
    char* abase = (char*)arena.p;
    b.d_obs = (double*)abase;
    b.d_eobs = (double*)(abase + b.b_obs);
    b.d_fwd = (double*)(abase + 2 * b.b_obs);
    b.d_bp = (short*)(abase + 2 * b.b_obs + b.b_fwd);
    b.d_lik = rt->buf("vit_lik").as<double>();
    return PS_OK;
}

// ---- stage: upload
static int upload(VitBatch& b) {
    PS_TRY(b.rt->up(b.d_regs, b.regs.data(), b.R * sizeof(VitReg)));
    PS_TRY(b.rt->up(b.d_posreg, b.pos_reg.data(), (size_t)b.ttot * sizeof(int)));
    for (int r = 0; r < b.R; r++) {
        const VitRegionH& g = b.regions[r];
        if (g.T && g.E) PS_TRY(b.rt->up(b.d_in + b.regs[r].in_off, g.obsin, (size_t)g.T * g.E * 4 * sizeof(double)));
    }
    return PS_OK;
}

// ---- stage: emissions.  Build 1 k_vit_obs_lds (up to 72 events, when its LDS can be had), 2 k_vit_obs<64>, 3 k_vit_obs<256>; a tap
// may ask for one that admits the batch's events, or bring the rows itself (ps_debug_viterbi_steps).  The profile's "viterbi"
// bracket opens here and closes in the tail.
static int emissions(VitBatch& b) {
    const bool lds_ok = b.maxE <= 72 && vit_obs_lds_ok();
    int build = lds_ok ? 1 : b.maxE <= 64 ? 2 : 3;
    if (b.tap && b.tap->obs_build) {
        build = b.tap->obs_build;
        if (build < 1 || build > 3 || (build == 1 && !lds_ok) || (build == 2 && b.maxE > 64))
            return fail(PS_ERR_BAD_ARG, "ViterbiMutate: the emission build asked for does not take this many events");
    }
    prof_begin(b.rt);
    if (b.tap && b.tap->obs_rows) {
        std::vector<double> eo(b.cells());
        for (size_t k = 0; k < eo.size(); k++) eo[k] = std::exp(b.tap->obs_rows[k]);
        PS_TRY(b.rt->up(b.d_obs, b.tap->obs_rows, eo.size() * sizeof(double)));
        PS_TRY(b.rt->up(b.d_eobs, eo.data(), eo.size() * sizeof(double)));
    } else {
        launch_vit_obs(b.rt, build, b.d_regs, b.d_posreg, b.d_in, b.ttot, b.maxE, b.d_obs, b.d_eobs);
    }
    return PS_OK;
}

// ---- stage: steps, and the final scores on their way back
static int steps(VitBatch& b) {
    PS_TRY(launch_vit_steps(b.rt, b.d_regs, b.R, b.d_obs, b.d_eobs, b.call.skip, b.call.stay, b.d_bp, b.d_fwd, b.d_lik, b.call.nkeep != 0));
    return b.rt->down(&b.lik, b.d_lik, (size_t)b.R * NS);
}

// ---- stage: tap.  The tables as the kernels left them: the forward vectors before k_vit_log overwrites them
static int tap_tables(VitBatch& b) {
    if (!b.tap) return PS_OK;
    PS_TRY(b.rt->down(&b.tap_obs, b.d_obs, b.cells()));
    PS_TRY(b.rt->down(&b.tap_bp, b.d_bp, b.cells()));
    if (b.call.nkeep > 0) PS_TRY(b.rt->down(&b.tap_fwd, b.d_fwd, b.cells()));
    return PS_OK;
}
static void tap_append(VitBatch& b) {   // (once the stream has been synchronised)
    VitTap* tap = b.tap;
    if (!tap) return;
    tap->obs.insert(tap->obs.end(), b.tap_obs, b.tap_obs + b.cells());
    tap->bp.insert(tap->bp.end(), b.tap_bp, b.tap_bp + b.cells());
    if (b.tap_fwd) tap->fwd.insert(tap->fwd.end(), b.tap_fwd, b.tap_fwd + b.cells());
    for (int r = 0; r < b.R; r++)   // (a region without positions keeps its zeros: k_vit_steps writes nothing for it)
        if (b.regions[r].T) std::copy(b.lik + (size_t)r * NS, b.lik + (size_t)(r + 1) * NS, tap->lik_final.end() - (size_t)(b.R - r) * NS);
}
static void tap_paths(VitBatch& b) {
    if (b.tap) for (int r = 0; r < b.R; r++) *(b.tap->paths.end() - b.R + r) = b.regions[r].paths;
}

// ---- stage: draw.  The uniform deviates of the stochastic back-traces are drawn on the host while the recursion runs: per region in
// the reference's call order (for each kept path, one per back-step, cpp/Viterbi.cpp:108) from the region's own generator.  Then
// the synchronisation that brings the final scores, and every region's start state from them.
static int draw(VitBatch& b) {
    const int nkeep = b.call.nkeep;
    if (nkeep > 0) {
        b.h_rand = (double*)b.rt->stage.alloc((size_t)nkeep * b.ttot * sizeof(double));
        if (!b.h_rand) return fail(PS_ERR_NOMEM, "hipHostMalloc (staging arena)");
        for (int r = 0; r < b.R; r++) b.regions[r].draw(b.regions[r].rng, b.h_rand + (size_t)nkeep * b.regs[r].t_off, (size_t)nkeep * b.regions[r].T);
    }
    PS_HIP(hipStreamSynchronize(b.rt->stream));
    tap_append(b);
    b.starts.assign(b.R, 0);
    for (int r = 0; r < b.R; r++) b.starts[r] = (int)(std::max_element(b.lik + (size_t)r * NS, b.lik + (size_t)(r + 1) * NS) - (b.lik + (size_t)r * NS));
    return PS_OK;
}

// ---- stage: the deterministic tail (nkeep == 0).  A back-pointer of -1 on the path (a dead max-plus row)
// refuses the whole call
static int follow_tail(VitBatch& b) {
    short* bp = nullptr;
    PS_TRY(b.rt->down(&bp, b.d_bp, b.cells()));
    PS_HIP(hipStreamSynchronize(b.rt->stream));
    prof_end(b.rt, "viterbi", (double)b.ttot * NS * (8.0 * b.maxE + 8 + 2));
    for (int r = 0; r < b.R; r++) {
        VitRegionH& g = b.regions[r];
        if (!g.T) continue;
        std::vector<int> p(g.T);
        const int64_t dead = vit_follow_bp(bp, b.regs[r].t_off, g.T, NS, b.starts[r], p.data());
        if (dead >= 0) {
            for (int q = 0; q < b.R; q++) b.regions[q].paths.clear();
            return fail(PS_ERR_BAD_ARG, std::string(b.call.who) + ": " + (g.index >= 0 ? "region " + std::to_string(g.index) + ": " : std::string()) +
                                            "no state is reachable at kept position " + std::to_string(dead) +
                                            " (every emission there is -inf or below -1e300, or the running scores have passed -1e300)");
        }
        g.paths.assign(p.begin(), p.end());
    }
    tap_paths(b);
    return PS_OK;
}

// ---- stage: the stochastic tail (nkeep > 0).  k_vit_log, then nkeep back-traces per region
static int trace_tail(VitBatch& b) {
    Runtime* rt = b.rt;
    const int nkeep = b.call.nkeep;
    std::vector<double> att(nkeep);
    for (int k = 0; k < nkeep; k++) att[k] = b.call.mmin + (b.call.mmax - b.call.mmin) * k / (double)nkeep;
    PS_TRY(rt->up(rt->buf("vit_att").p, att.data(), nkeep * sizeof(double)));
    PS_TRY(rt->up(rt->buf("vit_start").p, b.starts.data(), b.R * sizeof(int)));
    PS_HIP(hipMemcpyAsync(rt->buf("vit_rnd").p, b.h_rand, (size_t)nkeep * b.ttot * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    PS_TRY(launch_vit_trace(rt, b.d_regs, b.R, b.ttot, nkeep, b.d_fwd, rt->buf("vit_start").as<int>(), b.call.skip, b.call.stay, rt->buf("vit_att").as<double>(),
                            rt->buf("vit_rnd").as<double>(), rt->buf("vit_path").as<short>()));
    prof_end(rt, "viterbi", (double)b.ttot * NS * (8.0 * b.maxE + 8 + 2 + 8 + 8.0 * nkeep));
    short* hp = nullptr;
    PS_TRY(rt->down(&hp, rt->buf("vit_path").p, (size_t)nkeep * b.ttot));
    PS_HIP(hipStreamSynchronize(rt->stream));
    for (int r = 0; r < b.R; r++) {
        const short* rp = hp + (size_t)nkeep * b.regs[r].t_off;
        b.regions[r].paths.assign(rp, rp + (size_t)nkeep * b.regions[r].T);
    }
    tap_paths(b);
    return PS_OK;
}

int viterbi_batch(Runtime* rt, const VitCall& call, VitRegionH* regs, size_t n) {
    VitBatch b(rt, call, regs, n);
    plan(b);
    if (b.ttot <= 0) return PS_OK;
    if (b.maxE > 256) return fail(PS_ERR_UNSUPPORTED, "ViterbiMutate: more than 256 events");
    PS_TRY(place(b));
    PS_TRY(upload(b));
    PS_TRY(emissions(b));
    PS_TRY(steps(b));
    PS_TRY(tap_tables(b));
    PS_TRY(draw(b));
    return call.nkeep == 0 ? follow_tail(b) : trace_tail(b);
}

}  // namespace ps
