// ps_own.cpp — the calls that align every event of an AlignData to its own sequence, forward only: ScoreAlignments
// (cpp/MakeMutations.cpp:148-195), ps_align_stats, ps_kmer_stats, ps_move_stats and — a chain of its own below, posterior():
// sum-product fills instead of a realignment — ps_posterior_stats, for several AlignData in lock-step (independent regions in one
// launch chain).  One request record per AlignData (OwnReq, ps_host.h) and one chain, own_forward: the cuts of a call that does not
// fit this runtime's share, the batch, the optional realignment (with k_move_stats inside it for ps_move_stats, whose outputs are
// placed before it), the tail the kinds differ in, the scores.  Batch and realign() are
// in ps_host.cpp, struct Align in ps_align.cpp, the kernels of the three reductions in ps_stats.hip.
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

// The descriptors of k_align_stats and k_kmer_stats for reqs[0 .. n - 1], whose events are the jobs of `b` in order: one StatJob per
// event, one StatRegion per AlignData.  kmer: the events' group ids and the numbers of groups count; the regions' table rows follow
// each other.  Returns the levels of all events.
static double stat_descriptors(const OwnReq* reqs, size_t n, const Batch& b, bool kmer, std::vector<StatJob>* sj, std::vector<StatRegion>* sr, int* maxE) {
    sj->assign(b.jobs.size(), StatJob());
    sr->assign(n, StatRegion());
    *maxE = 0;
    double levels = 0;
    size_t q = 0;
    int tab = 0;
    for (size_t k = 0; k < n; k++) {
        const Align* a = reqs[k].a;
        StatRegion& r = (*sr)[k];
        r.job0 = (int)q; r.njobs = a->E; r.ngroups = kmer ? reqs[k].ngroups : 0; r.tab0 = tab;
        tab += r.ngroups;
        *maxE = std::max(*maxE, a->E);
        for (int e = 0; e < a->E; e++, q++) {
            const JobD& j = b.jobs[q];
            StatJob& s = (*sj)[q];
            s.ra = j.ra; s.mean = a->d_mean + a->off[e]; s.stdv = a->d_stdv + a->off[e]; s.model = a->d_model + (size_t)e * 6 * NS;
            s.st = j.st; s.n = j.n0; s.S = j.C;
            s.grp = kmer ? reqs[k].group[e] : 0; s.pad = 0;
            levels += j.n0;
        }
    }
    return levels;
}

// bytes of the tables of a k-mer call (48 KiB per group), and the most groups of one AlignData
static size_t table_bytes(const OwnReq* reqs, size_t n, int* maxG = nullptr) {
    size_t rows = 0;
    for (size_t k = 0; k < n; k++) { rows += (size_t)reqs[k].ngroups; if (maxG) *maxG = std::max(*maxG, reqs[k].ngroups); }
    return rows * NS * sizeof(ps_kmer_cell);
}

// The tail of the two statistics: the descriptors in through "astats_in"; one launch of k_align_stats or k_kmer_stats over the refs
// the backtrace just wrote (re) or the handles hold; in "astats" the records or tables and, behind them, the scores (re), back in
// one copy.  *best: the scores in that copy, null without a realignment.
static int stats_tail(Runtime* rt, bool kmer, bool re, const Batch& b, OwnReq* reqs, size_t n, double** best) {
    const size_t nj = b.jobs.size();
    std::vector<StatJob> sj;
    std::vector<StatRegion> sr;
    int maxE = 0, maxG = 0;
    const double levels = stat_descriptors(reqs, n, b, kmer, &sj, &sr, &maxE);
    const size_t out_main = kmer ? table_bytes(reqs, n, &maxG) : nj * sizeof(ps_event_stats);
    const double bytes = (kmer ? 24.0 : 16.0) * levels + (double)out_main;
    const size_t in_jobs = nj * sizeof(StatJob), in_bytes = in_jobs + sr.size() * sizeof(StatRegion);
    const size_t out_bytes = out_main + (re ? nj * sizeof(double) : 0);
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(in_bytes));
    PS_TRY(dout.ensure(out_bytes));
    PS_TRY(rt->up(din.p, sj.data(), in_jobs));
    PS_TRY(rt->up((char*)din.p + in_jobs, sr.data(), sr.size() * sizeof(StatRegion)));
    const StatRegion* dsr = (const StatRegion*)((char*)din.p + in_jobs);
    if (kmer) PS_TRY(launch_kmer_stats(rt, din.as<StatJob>(), dsr, (int)sr.size(), maxG, bytes, dout.as<ps_kmer_cell>()));
    else PS_TRY(launch_align_stats(rt, din.as<StatJob>(), dsr, (int)sr.size(), maxE, bytes, dout.as<ps_event_stats>()));
    if (re) PS_TRY(launch_gather_best(rt, b.d, (double*)((char*)dout.p + out_main)));
    void* back = nullptr;
    PS_TRY(rt->down(&back, dout.p, out_bytes));
    PS_HIP(hipStreamSynchronize(rt->stream));
    for (size_t k = 0; k < n; k++) {
        if (kmer) memcpy(reqs[k].table, (const ps_kmer_cell*)back + (size_t)sr[k].tab0 * NS, (size_t)reqs[k].ngroups * NS * sizeof(ps_kmer_cell));
        else memcpy(reqs[k].stats, (const ps_event_stats*)back + sr[k].job0, (size_t)reqs[k].a->E * sizeof(ps_event_stats));
    }
    *best = re ? (double*)((char*)back + out_main) : nullptr;
    return PS_OK;
}

// ps_move_stats: k_move_stats runs INSIDE the realignment, between the walk and the kernel that overwrites the walk's records, so
// its descriptors (through "astats_in") and its outputs (in "astats": the records, the scores, then the per-level columns and step
// codes when a request wants them) are placed before realign() runs; no kernel of that chain touches either pool.
struct MovePlan {
    size_t nj = 0, levels = 0, sc_off = 0, col_off = 0, step_off = 0, out_bytes = 0;
    bool per_level = false;
    std::vector<size_t> lev_off;   // of every job in the per-level arrays
};
static int moves_place(Runtime* rt, Batch& b, const OwnReq* reqs, size_t n, MovePlan* mp) {
    mp->nj = b.jobs.size();
    std::vector<MoveJob> mj(mp->nj);
    std::vector<StatRegion> sr(n);
    int maxE = 0;
    for (size_t k = 0; k < n; k++) mp->per_level |= reqs[k].step || reqs[k].col;
    mp->lev_off.assign(mp->nj, 0);
    for (size_t q = 0; q < mp->nj; q++) { mp->lev_off[q] = mp->levels; mp->levels += (size_t)b.jobs[q].n0; }
    mp->sc_off = mp->nj * sizeof(ps_event_moves);
    mp->col_off = mp->sc_off + mp->nj * sizeof(double);
    mp->step_off = mp->col_off + (mp->per_level ? mp->levels * sizeof(int32_t) : 0);
    mp->out_bytes = mp->step_off + (mp->per_level ? mp->levels : 0);
    const size_t in_jobs = mp->nj * sizeof(MoveJob), in_bytes = in_jobs + n * sizeof(StatRegion);
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(in_bytes));
    PS_TRY(dout.ensure(mp->out_bytes));
    size_t q = 0;
    for (size_t k = 0; k < n; k++) {
        const Align* a = reqs[k].a;
        sr[k].job0 = (int)q; sr[k].njobs = a->E; sr[k].ngroups = 0; sr[k].tab0 = 0;
        maxE = std::max(maxE, a->E);
        for (int e = 0; e < a->E; e++, q++) {
            const JobD& j = b.jobs[q];
            MoveJob& m = mj[q];
            m.rec = (const long long*)j.rl; m.out = j.out; m.n = j.n0; m.pad = 0;
            m.col = reqs[k].col ? (int32_t*)((char*)dout.p + mp->col_off) + mp->lev_off[q] : nullptr;
            m.step = reqs[k].step ? (uint8_t*)dout.p + mp->step_off + mp->lev_off[q] : nullptr;
        }
    }
    PS_TRY(rt->up(din.p, mj.data(), in_jobs));
    PS_TRY(rt->up((char*)din.p + in_jobs, sr.data(), n * sizeof(StatRegion)));
    b.moves.jobs = din.as<MoveJob>();
    b.moves.regs = (const StatRegion*)((char*)din.p + in_jobs);
    b.moves.nregs = (int)n; b.moves.maxE = maxE;
    b.moves.out = dout.as<ps_event_moves>();
    b.moves.alg_bytes = (mp->per_level ? 13.0 : 8.0) * (double)mp->levels + (double)mp->sc_off;
    return PS_OK;
}
// and its tail: the scores behind the records, everything back in one copy, the requests' arrays filled
static int moves_tail(Runtime* rt, const Batch& b, const MovePlan& mp, OwnReq* reqs, size_t n, double** best) {
    DBuf& dout = rt->buf("astats");
    PS_TRY(launch_gather_best(rt, b.d, (double*)((char*)dout.p + mp.sc_off)));
    void* back = nullptr;
    PS_TRY(rt->down(&back, dout.p, mp.out_bytes));
    PS_HIP(hipStreamSynchronize(rt->stream));
    size_t q = 0;
    for (size_t k = 0; k < n; k++) {
        const Align* a = reqs[k].a;
        memcpy(reqs[k].moves, (const ps_event_moves*)back + q, (size_t)a->E * sizeof(ps_event_moves));
        for (int e = 0; e < a->E; e++, q++) {
            const size_t ne = (size_t)a->n[e];
            if (reqs[k].col && reqs[k].col[e]) memcpy(reqs[k].col[e], (const int32_t*)((const char*)back + mp.col_off) + mp.lev_off[q], ne * sizeof(int32_t));
            if (reqs[k].step && reqs[k].step[e]) memcpy(reqs[k].step[e], (const uint8_t*)back + mp.step_off + mp.lev_off[q], ne);
        }
    }
    *best = (double*)((char*)back + mp.sc_off);
    return PS_OK;
}

// ---- ps_posterior_stats: the band stage of the fills, k_post_fwd and k_post_bwd (ps_post.hip) over skewed {M, S} records in "rec";
// the descriptors through "astats_in"; in "astats" the records and, behind them, the per-level arrays, back in one copy.  No
// backtrace and no updaterefs: nothing of the handles changes.
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
static double post_cells(const Batch& b) {
    double t = 0;
    for (const JobD& j : b.jobs) t += (double)j.C * std::min<double>(2.0 * j.W + 1, j.n0);
    return t;
}
static int posterior(Runtime* rt, OwnReq* reqs, size_t n) {
    auto sub = [&](size_t k0, size_t k1) { return posterior(rt, reqs + k0, k1 - k0); };
    auto need = [&](size_t k) { return post_need(reqs[k].a, post_slots(guess_slots(reqs[k].a))); };
    if (n > 1 && over_share(n, 1, need)) return in_share_chunks(n, 1, need, sub);
    std::vector<JobSpec> specs;
    for (size_t k = 0; k < n; k++)
        for (int e = 0; e < reqs[k].a->E; e++) specs.push_back(reqs[k].a->job(e));
    if (specs.empty()) return PS_OK;
    Batch b;
    PS_TRY(b.build(rt, specs, 1, 0));
    {
        const int rc = post_place(rt, b, n > 1 ? PLAN_OVER_GUESS * share_cap(1) : share_cap(1), n > 1);
        if (rc == PS_SPLIT) return in_halves(n, sub);   // bands wider than guessed: two halves, one after the other
        PS_TRY(rc);
    }
    const size_t nj = b.jobs.size();
    bool per_level = false;
    for (size_t k = 0; k < n; k++) per_level |= reqs[k].emit != nullptr;
    std::vector<size_t> lev_off(nj, 0);
    size_t levels = 0;
    for (size_t q = 0; q < nj; q++) { lev_off[q] = levels; levels += (size_t)b.jobs[q].n0; }
    const size_t emit_off = nj * sizeof(ps_event_posterior), col_off = emit_off + (per_level ? levels * sizeof(double) : 0);
    const size_t out_bytes = col_off + (per_level ? levels * sizeof(double) : 0);   // what comes back; behind it the kernels' per-row sums
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(nj * sizeof(PostJob)));
    PS_TRY(dout.ensure(out_bytes + levels * 8 * sizeof(double)));
    std::vector<PostJob> pj(nj);
    size_t q = 0;
    for (size_t k = 0; k < n; k++)
        for (int e = 0; e < reqs[k].a->E; e++, q++) {
            pj[q].emit = reqs[k].emit ? (double*)((char*)dout.p + emit_off) + lev_off[q] : nullptr;
            pj[q].col = reqs[k].emit ? (double*)((char*)dout.p + col_off) + lev_off[q] : nullptr;
            pj[q].row = (double*)((char*)dout.p + out_bytes) + lev_off[q] * 8;
        }
    PS_TRY(rt->up(din.p, pj.data(), nj * sizeof(PostJob)));
    PS_TRY(launch_post(rt, b.d, b.P, din.as<PostJob>(), dout.as<ps_event_posterior>(), post_cells(b)));
    void* back = nullptr;
    PS_TRY(rt->down(&back, dout.p, out_bytes));
    PS_HIP(hipStreamSynchronize(rt->stream));
    q = 0;
    for (size_t k = 0; k < n; k++) {
        const Align* a = reqs[k].a;
        memcpy(reqs[k].post, (const ps_event_posterior*)back + q, (size_t)a->E * sizeof(ps_event_posterior));
        for (int e = 0; e < a->E; e++, q++) {
            if (!reqs[k].emit || reqs[k].post[e].inert || !a->n[e]) continue;   // (an inert event's arrays were not written)
            const size_t ne = (size_t)a->n[e];
            if (reqs[k].emit[e]) memcpy(reqs[k].emit[e], (const double*)((const char*)back + emit_off) + lev_off[q], ne * sizeof(double));
            if (reqs[k].pcol[e]) memcpy(reqs[k].pcol[e], (const double*)((const char*)back + col_off) + lev_off[q], ne * sizeof(double));
        }
    }
    return PS_OK;
}

// ps_debug_posterior: the same chain for one event, then its records un-skewed (the band per column from the lb table, as debug_fill)
int debug_posterior(Runtime* rt, Align* a, int ev, double* main, double* stay) {
    const std::vector<JobSpec> specs(1, a->job(ev));
    Batch b;
    PS_TRY(b.build(rt, specs, 1, 0));
    PS_TRY(post_place(rt, b, share_cap(1), false));
    DBuf& din = rt->buf("astats_in");
    DBuf& dout = rt->buf("astats");
    PS_TRY(din.ensure(sizeof(PostJob)));
    PS_TRY(dout.ensure(128 + (size_t)a->n[ev] * 8 * sizeof(double)));
    const PostJob none = {nullptr, nullptr, (double*)((char*)dout.p + 128)};
    PS_TRY(rt->up(din.p, &none, sizeof(none)));
    PS_TRY(launch_post(rt, b.d, b.P, din.as<PostJob>(), dout.as<ps_event_posterior>(), post_cells(b)));
    const JobD& J = b.jobs[0];
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
    if (kind == OwnKind::Posterior) return posterior(rt, reqs, n);
    const bool kmer = kind == OwnKind::KmerStats;
    auto sub = [&](size_t k0, size_t k1) { return own_forward(rt, kind, re, reqs + k0, k1 - k0); };   // regions k0 .. k1 - 1 as a call of their own
    // a k-mer call whose tables exceed this runtime's share is cut between AlignData
    if (kmer && n > 1 && (double)table_bytes(reqs, n) > device_share_bytes()) return in_halves(n, sub);
    auto need = [&](size_t k) { return share_need(reqs[k].a, 1); };
    if (re && over_share(n, 1, need)) return in_share_chunks(n, 1, need, sub);   // more matrices than this runtime's share of the device
    std::vector<JobSpec> specs;
    for (size_t k = 0; k < n; k++)
        for (int e = 0; e < reqs[k].a->E; e++) specs.push_back(reqs[k].a->job(e));
    if (specs.empty()) {
        for (size_t k = 0; kmer && k < n; k++) memset(reqs[k].table, 0, (size_t)reqs[k].ngroups * NS * sizeof(ps_kmer_cell));
        return PS_OK;
    }
    Batch b;   // (also without a realignment: it puts every sequence's states on the device)
    PS_TRY(b.build(rt, specs, 1, 0));
    MovePlan mp;
    if (kind == OwnKind::MoveStats) PS_TRY(moves_place(rt, b, reqs, n, &mp));
    if (re) {
        const int rc = realign(rt, b, n > 1 ? PLAN_OVER_GUESS * device_share_bytes() : 0.0);
        if (rc == PS_SPLIT) return in_halves(n, sub);   // bands wider than share_need guessed: two halves, one after the other
        PS_TRY(rc);
        for (size_t k = 0; k < n; k++) reqs[k].a->host_refs_valid = false;
    }
    double* best = nullptr;
    if (kind == OwnKind::Score) PS_TRY(score_tail(rt, b, reqs, n, &best));
    else if (kind == OwnKind::MoveStats) PS_TRY(moves_tail(rt, b, mp, reqs, n, &best));
    else PS_TRY(stats_tail(rt, kmer, re, b, reqs, n, &best));
    size_t q = 0;
    for (size_t k = 0; best && k < n; k++)
        for (int e = 0; e < reqs[k].a->E; e++, q++)
            if (reqs[k].scores) reqs[k].scores[e] = std::max(best[q], 0.0);   // Alignment::getMax, cpp/Alignment.h:127-130
    if (kind == OwnKind::Score) score_likes(reqs, n);
    return PS_OK;
}

}  // namespace ps
