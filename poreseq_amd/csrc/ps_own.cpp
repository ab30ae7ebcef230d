// ps_own.cpp — the calls that align every event of an AlignData to its own sequence, forward only: ScoreAlignments
// (cpp/MakeMutations.cpp:148-195), ps_align_stats, ps_kmer_stats, ps_move_stats and ps_posterior_stats, for several AlignData in
// lock-step (independent regions in one launch chain).  One request record per AlignData (OwnReq, ps_host.h), one statement of
// where the statistics' outputs lie in "astats" (OwnPlan, ps_ownplan.h) and one chain, own_forward, in stages: cut (a call that does
// not fit this runtime's share), jobs, batch, plan, place, fills (the optional realignment, with k_move_stats inside it for
// ps_move_stats; sum-product fills for ps_posterior_stats), reduce, fetch, scatter.  Batch and realign() are in ps_host.cpp,
// struct Align in ps_align.cpp, the kernels of the three reductions in ps_stats.hip, those of the posterior call in ps_post.hip.
#include "ps_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ps {

// The scores of a batch's jobs, gathered into one array on the device and enqueued for one copy back (instead of one per AlignData)
int gather_best(Runtime* rt, const Batch& b, double** best) {
    DBuf& gb = rt->buf("best");
    PS_TRY(gb.ensure(b.jobs.size() * sizeof(double)));
    PS_TRY(launch_gather_best(rt, b.d, gb.as<double>()));
    return rt->down(best, gb.p, b.jobs.size());
}

// ScoreAlignments' tail: the scores through "best", ref_align / ref_like of the AlignData that want their likelihoods, one
// synchronisation; score_likes adds the likelihoods up once the scores are written
static int score_tail(Runtime* rt, const Batch& b, OwnReq* reqs, size_t n, double** best) {
    PS_TRY(gather_best(rt, b, best));
    for (size_t k = 0; k < n; k++) if (reqs[k].likes) PS_TRY(reqs[k].a->refs_to_host_async(rt));
    PS_HIP(hipStreamSynchronize(rt->stream));
    return PS_OK;
}
static void score_likes(OwnReq* reqs, size_t n) {
    if (std::none_of(reqs, reqs + n, [](const OwnReq& q) { return q.likes != nullptr; })) return;
    par_for((int)n, [&](int k) {
        Align* a = reqs[k].a;
        if (!reqs[k].likes) return;
        a->refs_finish();
        for (int e = 0; e < a->E; e++) accumulate_likes(a->h_ra.data() + a->off[e], a->h_rl.data() + a->off[e], a->n[e], (int)a->states.size(), reqs[k].likes);
    });
}

// ---- ps_posterior_stats' fills: the band stage, then k_post_fwd and k_post_bwd (ps_post.hip) over skewed {M, S} records in "rec".
// No backtrace and no updaterefs: nothing of the handles changes.
// bytes of the records of one AlignData at P slots per anti-diagonal: (n0 + C + 25) x P x 16 per event (matrix_cells, ps_plan.h)
static double post_need(const Align* a, int P) {
    double t = 0;
    for (int e = 0; e < a->E; e++) t += (double)matrix_cells((int64_t)a->n[e] + (int64_t)a->states.size() + 1, P) * sizeof(double2);
    return t;
}
static int post_slots(int footprint) { return (std::max(footprint, 1) + 63) / 64 * 64; }
// k_begin's inert latch, k_lb, k_lo and the 4-byte footprint read-back that sizes P; then the records placed.  PS_SPLIT (can_split)
// or PS_ERR_NOMEM when they exceed `cap` bytes; nothing of the fill was launched then, b.P holds the slots they need.
static int post_place(Runtime* rt, Batch& b, double cap, bool can_split) {
    PS_TRY(launch_begin(rt, b.d));
    PS_TRY(launch_lb(rt, b.d, 0, b.maxlbn));
    PS_TRY(launch_lo(rt, b.d, 1, b.maxS));
    int* w = nullptr;
    PS_TRY(rt->down(&w, b.d.maxw, (size_t)1));
    PS_HIP(hipStreamSynchronize(rt->stream));
    const int P = post_slots(*w);
    if (P > POST_MAX_SLOTS)
        return fail(PS_ERR_UNSUPPORTED, "posterior: band footprint of " + std::to_string(*w) + " rows on one anti-diagonal: more than one lane per row of one workgroup holds (" +
                                        std::to_string(POST_MAX_SLOTS) + "); realign_width up to " + std::to_string((POST_MAX_SLOTS - 1) / 2) + " fits for any input");
    int64_t tot = 0;
    for (JobD& j : b.jobs) { j.P = P; j.K = 0; j.mat_off[0] = tot + (int64_t)MAT_FRONT * P; tot += matrix_cells(j.S, P); }
    b.P = P; b.cells = tot;
    const double bytes = (double)tot * sizeof(double2);
    if (cap > 0 && bytes > cap) {
        if (can_split) return PS_SPLIT;
        return fail(PS_ERR_NOMEM, "posterior: the forward tables of this AlignData need " + std::to_string((size_t)(bytes / 1048576.0) + 1) + " MB at " + std::to_string(P) +
                                  " slots per anti-diagonal, this thread's share of the device is " + std::to_string((size_t)(cap / 1048576.0)) + " MB");
    }
    void *prec = nullptr, *pflg = nullptr;
    const int rc = ensure_matrix_pools(rt, b, (size_t)std::max<int64_t>(tot, 1) * sizeof(double2), 0, can_split, &prec, &pflg);
    if (rc == PS_ERR_NOMEM && can_split) return PS_SPLIT;
    PS_TRY(rc);
    PS_TRY(rt->up(rt->buf("jobs").p, b.jobs.data(), b.jobs.size() * sizeof(JobD)));   // JobD.P, JobD.mat_off
    b.d.rec = (double2*)prec; b.d.flg = nullptr;
    return PS_OK;
}

// ---- the chain.  One call, or one sub-batch of it, on its way through the stages below, which fill it in this order
struct OwnChain {
    Runtime* rt; OwnKind kind; bool re;
    OwnReq* r; size_t n;   // r[0 .. n - 1]
    OwnView view; OwnPlan plan;
    Batch b;     // (also without a realignment: it puts every sequence's states on the device)
    DBuf *din = nullptr, *dout = nullptr;   // "astats_in", "astats"
    const StatRegion* d_regs = nullptr;     // behind the job descriptors in "astats_in"
    char* back = nullptr;                   // the copy of "astats" on the host
    OwnChain(Runtime* rt_, OwnKind kind_, bool re_, OwnReq* r_, size_t n_) : rt(rt_), kind(kind_), re(re_), r(r_), n(n_) {
        view.kind = kind; view.re = re;
        for (size_t k = 0; k < n; k++) view.regs.push_back({r[k].a->E, r[k].ngroups, r[k].step || r[k].col || r[k].emit});
    }
    bool kmer() const { return kind == OwnKind::KmerStats; }
    bool moves() const { return kind == OwnKind::MoveStats; }
    bool post() const { return kind == OwnKind::Posterior; }
};
// the one walk over the events of r[0 .. n - 1], which are the jobs of the chain's batch in order: f(region k, event e, job q)
template <class F> static void for_each_job(const OwnReq* r, size_t n, F&& f) {
    for (size_t k = 0, q = 0; k < n; k++)
        for (int e = 0; e < r[k].a->E; e++, q++) f(k, e, q);
}

// ---- stage: place.  Both pools sized; through "astats_in" one descriptor per job (StatJob, MoveJob or PostJob) and, behind them, one
// StatRegion per AlignData (none for the posterior kernels), every address into "astats" from the plan.  Before the fills for every kind:
// k_move_stats runs INSIDE the realignment, between the walk and the kernel that overwrites its records; no kernel there touches either pool.
static int place(OwnChain& c) {
    const OwnPlan& p = c.plan;
    std::vector<StatJob> sj(c.moves() || c.post() ? 0 : p.nj);
    std::vector<MoveJob> mj(c.moves() ? p.nj : 0);
    std::vector<PostJob> pj(c.post() ? p.nj : 0);
    std::vector<StatRegion> sr(c.post() ? 0 : c.n);
    const size_t in_jobs = sj.size() * sizeof(StatJob) + mj.size() * sizeof(MoveJob) + pj.size() * sizeof(PostJob);
    c.din = &c.rt->buf("astats_in"); c.dout = &c.rt->buf("astats");
    PS_TRY(c.din->ensure(in_jobs + sr.size() * sizeof(StatRegion)));
    PS_TRY(c.dout->ensure(p.ensure_bytes));
    void* out = c.dout->p;
    for (size_t k = 0; k < sr.size(); k++) sr[k] = {p.job0[k], c.r[k].a->E, c.kmer() ? c.r[k].ngroups : 0, p.tab0[k]};
    for_each_job(c.r, c.n, [&](size_t k, int e, size_t q) {
        const OwnReq& r = c.r[k]; const Align* a = r.a; const JobD& j = c.b.jobs[q];
        if (c.post()) pj[q] = {r.emit ? p.level<double>(out, OO_EMIT, q) : nullptr, r.emit ? p.level<double>(out, OO_PCOL, q) : nullptr, p.level<double>(out, OO_ROW, q, 8)};
        else if (c.moves()) mj[q] = {(const long long*)j.rl, j.out, r.step ? p.level<uint8_t>(out, OO_STEP, q) : nullptr, r.col ? p.level<int32_t>(out, OO_COL, q) : nullptr, j.n0, 0};
        else sj[q] = {j.ra, a->d_mean + a->off[e], a->d_model + (size_t)e * 6 * NS, j.st, j.n0, j.C, a->d_stdv + a->off[e], c.kmer() ? r.group[e] : 0, 0};
    });
    PS_TRY(c.rt->up(c.din->p, c.post() ? (const void*)pj.data() : c.moves() ? (const void*)mj.data() : (const void*)sj.data(), in_jobs));
    if (!sr.empty()) PS_TRY(c.rt->up((char*)c.din->p + in_jobs, sr.data(), sr.size() * sizeof(StatRegion)));
    c.d_regs = (const StatRegion*)((char*)c.din->p + in_jobs);
    if (c.moves()) {
        MoveRun& m = c.b.moves;
        m.jobs = c.din->as<MoveJob>(); m.regs = c.d_regs; m.nregs = (int)c.n; m.maxE = p.maxE;
        m.out = p.item<ps_event_moves>(out, OO_MAIN); m.alg_bytes = p.alg_bytes;
    }
    return PS_OK;
}

// ---- stage: fills.  PS_SPLIT when the bands came out wider than the cut guessed; nothing of the fill was launched then.  A
// realignment of one region is never split (cap 0); a lone posterior region gets the whole share and is refused beyond it.
// host_refs_valid goes only after a realignment: the posterior fills change nothing of the handles.
static int fills(OwnChain& c) {
    if (c.post()) {
        PS_TRY(post_place(c.rt, c.b, c.n > 1 ? PLAN_OVER_GUESS * share_cap(1) : share_cap(1), c.n > 1));
        return launch_post(c.rt, c.b.d, c.b.P, c.din->as<PostJob>(), c.plan.item<ps_event_posterior>(c.dout->p, OO_MAIN), c.plan.alg_bytes);
    }
    if (!c.re) return PS_OK;
    PS_TRY(realign(c.rt, c.b, c.n > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0));
    for (size_t k = 0; k < c.n; k++) c.r[k].a->host_refs_valid = false;
    return PS_OK;
}

// ---- stage: reduce.  One launch of k_align_stats or k_kmer_stats over the refs the backtrace just wrote or the handles hold
// (k_move_stats ran inside the realignment, the posterior kernels are their own reduction), and the scores behind the records
static int reduce(OwnChain& c) {
    const OwnPlan& p = c.plan;
    void* out = c.dout->p;
    if (c.kmer()) PS_TRY(launch_kmer_stats(c.rt, c.din->as<StatJob>(), c.d_regs, (int)c.n, p.maxG, p.alg_bytes, p.item<ps_kmer_cell>(out, OO_MAIN)));
    else if (c.kind == OwnKind::AlignStats) PS_TRY(launch_align_stats(c.rt, c.din->as<StatJob>(), c.d_regs, (int)c.n, p.maxE, p.alg_bytes, p.item<ps_event_stats>(out, OO_MAIN)));
    if (p.bytes[OO_SCORES]) PS_TRY(launch_gather_best(c.rt, c.b.d, p.item<double>(out, OO_SCORES)));
    return PS_OK;
}

// ---- stages: fetch, one copy and one synchronisation, and scatter: every output of the plan that a caller wants goes to its array
static int fetch(OwnChain& c) {
    PS_TRY(c.rt->down((void**)&c.back, c.dout->p, c.plan.back_bytes));
    PS_HIP(hipStreamSynchronize(c.rt->stream));
    return PS_OK;
}
static void scatter(OwnChain& c) {
    const OwnPlan& p = c.plan;
    const size_t rec = own_out_elem(c.kind, OO_MAIN);
    for (size_t k = 0; k < c.n; k++) {
        const OwnReq& r = c.r[k];
        void* host = c.kmer() ? (void*)r.table : c.moves() ? (void*)r.moves : c.post() ? (void*)r.post : (void*)r.stats;
        const size_t i0 = c.kmer() ? (size_t)p.tab0[k] * NS : (size_t)p.job0[k], cnt = c.kmer() ? (size_t)r.ngroups * NS : (size_t)r.a->E;
        memcpy(host, p.item<char>(c.back, OO_MAIN, i0 * rec), cnt * rec);
    }
    if (!p.per_level) return;
    for_each_job(c.r, c.n, [&](size_t k, int e, size_t q) {
        const OwnReq& r = c.r[k]; const size_t ne = (size_t)r.a->n[e];
        auto put = [&](void* to, OwnOut o) { const size_t el = own_out_elem(c.kind, o); if (to) memcpy(to, p.level<char>(c.back, o, q, el), ne * el); };
        if (r.col) put(r.col[e], OO_COL);
        if (r.step) put(r.step[e], OO_STEP);
        if (!r.emit || r.post[e].inert || !ne) return;   // (an inert event's arrays were not written)
        put(r.emit[e], OO_EMIT);
        put(r.pcol[e], OO_PCOL);
    });
}

// ps_debug_posterior: the same chain for one event, then its records un-skewed (the band per column from the lb table, as debug_fill)
int debug_posterior(Runtime* rt, Align* a, int ev, double* main, double* stay) {
    const std::vector<JobSpec> specs(1, a->job(ev));
    Batch b;
    PS_TRY(b.build(rt, specs, 1, 0));
    PS_TRY(post_place(rt, b, share_cap(1), false));
    const JobD& J = b.jobs[0];
    OwnView view;   // a one-event call without per-level arrays
    view.kind = OwnKind::Posterior; view.regs.push_back({1, 0, false}); view.jobs.push_back({J.n0, J.C, J.W});
    const OwnPlan plan = lay_out(view);
    DBuf &din = rt->buf("astats_in"), &dout = rt->buf("astats");
    PS_TRY(din.ensure(sizeof(PostJob)));
    PS_TRY(dout.ensure(plan.ensure_bytes));
    const PostJob none = {nullptr, nullptr, plan.level<double>(dout.p, OO_ROW, 0, 8)};
    PS_TRY(rt->up(din.p, &none, sizeof(none)));
    PS_TRY(launch_post(rt, b.d, b.P, din.as<PostJob>(), plan.item<ps_event_posterior>(dout.p, OO_MAIN), plan.alg_bytes));
    const int n0 = J.n0, C = J.C, P = J.P;
    const size_t ld = (size_t)C + 1, tot = ((size_t)n0 + 1) * ld;
    const double nan = std::nan("");
    for (size_t k = 0; k < tot; k++) { main[k] = nan; if (stay) stay[k] = nan; }
    for (int i = 0; i <= n0; i++) { main[(size_t)i * ld] = 0.0; if (stay) stay[(size_t)i * ld] = 0.0; }   // the blank column
    ps_event_posterior rec0;
    std::vector<int> lb(J.lbn);
    std::vector<double2> rec((size_t)J.S * P);
    PS_HIP(hipMemcpyAsync(&rec0, dout.p, sizeof(rec0), hipMemcpyDeviceToHost, rt->stream));
    PS_HIP(hipMemcpyAsync(lb.data(), b.d.lb + J.lb_off, J.lbn * sizeof(int), hipMemcpyDeviceToHost, rt->stream));
    PS_HIP(hipMemcpyAsync(rec.data(), b.d.rec + J.mat_off[0], rec.size() * sizeof(double2), hipMemcpyDeviceToHost, rt->stream));
    PS_HIP(hipStreamSynchronize(rt->stream));
    if (rec0.inert) return PS_OK;
    for (int c = 1; c <= C; c++) {
        const int v = lb[c];
        const int ce = std::min(std::max(v < 0 ? 1 : v, 1), n0);
        const int i0 = std::max(1, ce - J.W), i1 = std::min(n0, ce + J.W);
        for (int i = i0; i <= i1; i++) {
            const size_t to = (size_t)i * ld + c, at = (size_t)(i + c) * P + (i % P);
            main[to] = rec[at].x;
            if (stay) stay[to] = rec[at].y;
        }
    }
    return PS_OK;
}

int own_forward(Runtime* rt, OwnKind kind, bool re, OwnReq* reqs, size_t n) {
    OwnChain c(rt, kind, re, reqs, n);
    auto sub = [&](size_t k0, size_t k1) { return own_forward(rt, kind, re, reqs + k0, k1 - k0); };   // regions k0 .. k1 - 1 as a call of their own
    // ---- cut.  A k-mer call whose tables exceed this runtime's share is halved between AlignData; fills — a realignment only when
    // it runs — are cut to the share on a guess of their matrices (share_need) or forward tables (post_need)
    if (c.kmer() && n > 1 && (double)lay_out(c.view).bytes[OO_MAIN] > device_share_bytes()) return in_halves(n, sub);
    auto need = [&](size_t k) { return c.post() ? post_need(reqs[k].a, post_slots(guess_slots(reqs[k].a))) : share_need(reqs[k].a, 1); };
    if ((re || c.post()) && over_share(n, 1, need)) return in_share_chunks(n, 1, need, sub);
    // ---- jobs, batch
    std::vector<JobSpec> specs;
    for_each_job(reqs, n, [&](size_t k, int e, size_t) { specs.push_back(reqs[k].a->job(e)); });
    if (specs.empty()) {   // (the tables of a k-mer call without events: zeroed here)
        for (size_t k = 0; c.kmer() && k < n; k++) memset(reqs[k].table, 0, (size_t)reqs[k].ngroups * NS * sizeof(ps_kmer_cell));
        return PS_OK;
    }
    PS_TRY(c.b.build(rt, specs, 1, 0));
    // ---- plan, place: the statistics' outputs in "astats" (ScoreAlignments has none there: its scores go through "best")
    if (kind != OwnKind::Score) {
        for (const JobD& j : c.b.jobs) c.view.jobs.push_back({j.n0, j.C, j.W});
        c.plan = lay_out(c.view);
        PS_TRY(place(c));
    }
    if (const int rc = fills(c)) return rc == PS_SPLIT ? in_halves(n, sub) : rc;   // bands wider than guessed: two halves, one after the other
    double* best = nullptr;
    if (kind == OwnKind::Score) PS_TRY(score_tail(rt, c.b, reqs, n, &best));
    else {
        PS_TRY(reduce(c)); PS_TRY(fetch(c)); scatter(c);
        if (c.plan.bytes[OO_SCORES]) best = c.plan.item<double>(c.back, OO_SCORES);
    }
    if (best) for_each_job(reqs, n, [&](size_t k, int e, size_t q) { if (reqs[k].scores) reqs[k].scores[e] = std::max(best[q], 0.0); });   // Alignment::getMax, cpp/Alignment.h:127-130
    if (kind == OwnKind::Score) score_likes(reqs, n);
    return PS_OK;
}

}  // namespace ps
